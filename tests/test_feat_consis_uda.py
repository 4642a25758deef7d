"""The feature-consistency loss of the `isr_no_fusion` route of train type 'cs2dsec_image+events' (encoder_decoder.py:822-823,
:833-848; dacs.py:186-195, :509-511, :840-842): the segmentor's `decode.loss_feat_consis` and its gradient against torch, the DACS log
keys / values, and on the GPU the whole step against the reference's own code (tests/golden/dacs_step_nofusion.npz, written by
tests/golden/make_golden_featconsis.py) and graph replay against eager.  The fixture's 512 x 512 step is compared on the GPU only (as every
step fixture of the suite); the emulator runs the same route on the small model and checks the fixture's log KEYS."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import DACS_CH, DACS_DIMS, DACS_SEG_SCALE, dacs_batch, sample_grad, seeded_fill  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
import test_dacs as TD  # noqa: E402
from cmda_amd import ops  # noqa: E402
from cmda_amd.registry import build_segmentor, build_train_model  # noqa: E402
from conftest import assert_close, check_le  # noqa: E402

TT = 'cs2dsec_image+events'
SEEDS = dict(student=171, teacher=172, generator=173)   # make_golden_featconsis.SEEDS
FP_N = 12
DIRECT = [['leftdown', 'leftup'], ['rightdown', 'rightup']]
SMALL = dict(dims=[32, 64, 160, 256], ch=64)
FC_KEYS = ['decode.loss_feat_consis', 'mix.decode.loss_feat_consis']
CASES = dict(isr=(2.0, 0.4, 2), default=(2.0, -1, 1), events=(-1.0, 0.4, 1))   # make_golden_featconsis.CASES


def golden(name='dacs_step_nofusion.npz'):
    return {k: (v.tolist() if v.dtype.kind == 'U' else torch.from_numpy(v)) for k, v in np.load(os.path.join(HERE, 'golden', name)).items()}


def make_cfg(dims, ch, train_type=TT, generator=True, **uda):
    cfg = TD.make_cfg(dims, ch, generator=generator, train_type=train_type)
    cfg['uda'].update(uda)
    return cfg


def small_segmentor(tgt, seed=61):
    m = build_segmentor(make_cfg(**SMALL)['model'])
    seeded_fill(m, seed)
    return m.to(tgt.device).train()


def seg_inputs(tgt, B=1, H=32, W=32):
    src, _ = TD.make_batch(B, H, W)
    return {'image': tgt.to(src['image']), 'events': tgt.to(src['img_self_res'])}, tgt.to(src['label'])


def torch_term(feats, lam):
    """lam * sum_i mse_loss(f_image[i], f_events[i].detach()) in float64 on the returned features, and its gradient per level"""
    fa = [f[0].detach().cpu().double().requires_grad_(True) for f in feats['f_image']]
    fb = [f[0].detach().cpu().double() for f in feats['f_events']]
    loss = sum(lam * F.mse_loss(a, b) for a, b in zip(fa, fb))
    loss.backward()
    return loss.detach(), [a.grad for a in fa]


# ---------------------------------------------------------------------------------------------------------------------------
# segmentor (emulator and GPU)
def test_forward_train_returns_the_term(tgt):
    rt.set_compute_dtype(torch.float32)
    m = small_segmentor(tgt)
    inputs, gt = seg_inputs(tgt)
    cfg = dict(TD.FCFG, no_fusion=True, lambda_feature_consistency=0.4)
    out, _ = m.forward_train(inputs, gt, return_feat=True, cfg=cfg)
    assert 'decode.loss_feat_consis' in out and out['decode.loss_feat_consis'].shape == ()
    ref, _ = torch_term(out['features'], 0.4)
    check_le('decode.loss_feat_consis vs torch mse_loss on the returned features, rel',
             abs(out['decode.loss_feat_consis'].item() - ref.item()) / ref.item(), 1e-5)
    assert ref.item() > 0
    # the fusion route of the same model, and the same cfg under another train type, have no such term
    out, _ = m.forward_train(inputs, gt, cfg=dict(TD.FCFG))
    assert 'decode.loss_feat_consis' not in out
    assert not m._feat_consis_on(dict(TD.FCFG, no_fusion=False)) and not m._feat_consis_on(None)
    with torch.device('meta'):
        other = build_segmentor(make_cfg(**SMALL, train_type='cs2dsec_image+events_together')['model'])
    assert not other._feat_consis_on(cfg)


def test_forward_train_gradient_of_the_term(tgt):
    """parameter gradients of (loss_seg + loss_feat_consis).backward() at lambda 0.4 minus those at lambda 0: in the image encoder,
    `backbone_image.bwd` fed with torch's gradient of the term; the event encoder (the ISR features are detached) and the head see none
    of it.  Bound of the difference: the three back-propagations carry fp32 round-off of their own tensors, each held to 3e-5 of the
    tensor's maximum at kernel level (tests/test_kernels.py), so the difference is held to 3e-5 of the three maxima added up."""
    rt.set_compute_dtype(torch.float32)
    m = small_segmentor(tgt)
    inputs, gt = seg_inputs(tgt)
    grads, feats = {}, None
    for lam in (0.0, 0.4):
        for p in m.parameters():
            p.grad = None
        out, _ = m.forward_train(inputs, gt, return_feat=True, cfg=dict(TD.FCFG, no_fusion=True, lambda_feature_consistency=lam))
        (out['decode.loss_seg'] + out['decode.loss_feat_consis']).backward()
        grads[lam] = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
        feats = out['features']
        if lam == 0.0:
            assert float(out['decode.loss_feat_consis']) == 0.0
    assert grads[0.0].keys() == grads[0.4].keys()
    _, dterm = torch_term(feats, 0.4)
    for p in m.parameters():
        p.grad = None
    _, sv = m.backbone_image.fwd(inputs['image'], save=True)
    with ops.backward_scope():
        m.backbone_image.bwd(sv, [tgt.to(d.float().contiguous()) for d in dterm])
        rt.join_lanes('wgrad')
    direct = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    assert direct and all(k.startswith('backbone_image.') for k in direct)
    worst, moved = 0.0, 0
    for k, g4 in grads[0.4].items():
        g0 = grads[0.0][k]
        if k.startswith('backbone_image.'):
            d = direct[k]
            scale = g4.abs().max().item() + g0.abs().max().item() + d.abs().max().item()
            worst = max(worst, ((g4 - g0) - d).abs().max().item() / (scale + 1e-30))
            if d.abs().max().item() > 0:   # (a few are exactly zero: the key bias, which the soft-max does not see)
                moved += 1
                assert (g4 - g0).abs().max().item() > 0, f'{k}: the term does not reach this gradient'
        else:   # identical up to the order of fp32 atomics in the weight-gradient kernels (run-to-run round-off, 1e-5 of the maximum)
            assert_close(g4, g0, 1e-5, name=f'{k} lambda 0.4 vs 0')
    assert moved > len(direct) // 2
    check_le('image-encoder gradient difference (lambda 0.4 - 0) vs backbone_image.bwd of the torch gradient', worst, 3e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# DACS on the small model (emulator and GPU)
def small_dacs(tgt, case, train_type=TT, **uda):
    thres, lam, _ = CASES[case]
    dacs = build_train_model(make_cfg(**SMALL, train_type=train_type, isr_no_fusion=True, lambda_feature_consistency=lam, **uda))
    dacs.random_choice_thres = thres
    seeded_fill(dacs.model, 7), seeded_fill(dacs.ema_model, 8), seeded_fill(dacs.cyclegan_itrd2en, 9)
    return dacs.to(tgt.device).train()


def small_iteration(tgt, dacs, B=1):
    src, tg = TD.make_batch(B, 64, 64)
    torch.manual_seed(11), random.seed(11), np.random.seed(11)
    lv = dacs(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
    return {k: float(v) for k, v in lv.items()}


def test_dacs_log_keys_and_values_follow_the_fixture_cases(tgt):
    rt.set_compute_dtype(torch.float32)
    g = golden()
    lvs = {}
    for case in (CASES if tgt.kind == 'gpu' else ('isr', 'events')):   # (an emulated iteration takes a minute: `default` below)
        dacs = small_dacs(tgt, case)
        lv = lvs[case] = small_iteration(tgt, dacs)
        assert sorted(k for k in lv if k != 'loss') == sorted(g[f'{case}.it0.log_keys']), f'{case}: log keys'   # (train_step drops 'loss')
        assert all(np.isfinite(v) for v in lv.values())
        if case == 'events':
            assert not any('feat_consis' in k for k in lv) and lv['loss'] == lv['mix.decode.loss_seg']
            continue
        # _parse_losses of the mixed step: every '*loss*' entry summed, in fp32
        check_le(f'{case} loss vs mix loss_seg + loss_feat_consis, rel (two fp32 ulps)',
                 abs(lv['loss'] - lv['mix.decode.loss_seg'] - lv['mix.decode.loss_feat_consis']) / lv['loss'], 2.0 ** -22)
        # the source pass's value against torch on that pass's own features (recomputed: same weights, no stochastic layer)
        with torch.no_grad():
            src, _ = TD.make_batch(1, 64, 64)
            fa, _ = dacs.model.backbone_image.fwd(tgt.to(src['image']), save=False)
            fb, _ = dacs.model.backbone_events.fwd(tgt.to(src['img_self_res']), save=False)
        lam = 0.4 if case == 'isr' else 0.25
        ref = sum(lam * F.mse_loss(a[0].cpu().double(), b[0].cpu().double()) for a, b in zip(fa, fb)).item()
        check_le(f'{case} decode.loss_feat_consis vs torch, rel', abs(lv['decode.loss_feat_consis'] - ref) / ref, 1e-5)
    # the key at -1, or absent, is 0.25 and reaches the student's cfg on the ISR route only; the same keys as the explicit value's
    assert g['default.it0.log_keys'] == g['isr.it0.log_keys']
    for uda in (dict(lambda_feature_consistency=-1), {}):
        with torch.device('meta'):
            d = build_train_model(make_cfg(**SMALL, isr_no_fusion=True, **uda))
        assert d._cfg_student(False)['lambda_feature_consistency'] == 0.25 and d._cfg_student(False)['no_fusion']
        assert not d._cfg_student(True).get('no_fusion')
    if 'default' not in lvs:
        return
    # the same weights and inputs: the values differ by the lambdas only, 0.25 (key at -1) against 0.4
    for k in FC_KEYS:
        check_le(f'{k}: default / explicit lambda', abs(lvs['default'][k] / lvs['isr'][k] - 0.25 / 0.4), 1e-5)
    for k in ('decode.loss_seg', 'mix.decode.loss_seg'):   # (the cross-entropy sums end in fp32 atomics: equal up to their order)
        check_le(f'{k}: default vs explicit lambda, rel', abs(lvs['default'][k] - lvs['isr'][k]) / lvs['isr'][k], 1e-6)


def test_other_train_types_have_no_such_term():
    """the flag and the key set under every other train type: the student's cfg never switches the term on, on either choice"""
    for tt in ('cs2dsec_image+events_together', 'cs2dz_image+raw-isr', 'cs2dz_image+raw-isr_split'):
        with torch.device('meta'):
            other = build_train_model(make_cfg(**SMALL, train_type=tt, generator=False, isr_no_fusion=True, lambda_feature_consistency=0.4))
        for use_events in (False, True):
            assert not other.model._feat_consis_on(other._cfg_student(use_events))
        assert not other.model._feat_consis_on(dict(no_fusion=True, lambda_feature_consistency=0.4))
    with torch.device('meta'):
        ours = build_train_model(make_cfg(**SMALL, isr_no_fusion=True))
        off = build_train_model(make_cfg(**SMALL))
    assert ours.model._feat_consis_on(ours._cfg_student(False)) and not ours.model._feat_consis_on(ours._cfg_student(True))
    assert not off.model._feat_consis_on(off._cfg_student(False))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the step against the reference's own code
def _gpu():
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    return Target('gpu')


def _fp_rel(got, ref):
    return max((got[:-2] - ref[:-2]).abs().max().item() / (ref[:-2].abs().max().item() + 1e-12),
               (got[-2:] - ref[-2:]).abs().max().item() / (ref[-1].abs().item() + 1e-12))


LOSS_KEYS = ['decode.loss_seg', 'decode.acc_seg', 'decode.loss_feat_consis', 'mix.decode.loss_seg', 'mix.decode.acc_seg',
             'mix.decode.loss_feat_consis', 'loss']


@pytest.mark.gpu
@pytest.mark.parametrize('case,mode', [('isr', 'f32'), ('isr', 'x3'), ('default', 'f32'), ('events', 'f32')])
def test_nofusion_step_against_reference_fixture_gpu(case, mode):
    """train_step on one 512 x 512 pair with the reference's recorded draws injected, FlatAdamW between the iterations: log keys, the
    losses (the consistency term included), the mixed tensors, gradient and EMA fingerprints, with the bounds
    tests/test_fdist.py::test_dacs_fdist_step_against_reference_fixture_gpu applies to the same quantities in the exact and the
    split-bf16 mode"""
    from cmda_amd.optim import FlatAdamW
    _gpu()
    thres, lam, iters = CASES[case]
    g = golden()
    src, tg = dacs_batch()
    exact = mode == 'f32'
    rt.set_compute_dtype(torch.float32)
    rt.set_gemm_x3(mode == 'x3')
    dacs = None
    try:
        dacs = build_train_model(make_cfg(DACS_DIMS, DACS_CH, isr_no_fusion=True, lambda_feature_consistency=lam))
        dacs.random_choice_thres = thres
        seeded_fill(dacs.model, SEEDS['student'])
        seeded_fill(dacs.ema_model, SEEDS['teacher'])
        seeded_fill(dacs.cyclegan_itrd2en, SEEDS['generator'])
        with torch.no_grad():
            dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
        dacs = dacs.to('cuda:0').train()
        opt = FlatAdamW(dacs.model, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
        row = {k: i for i, k in enumerate(g['param_names'])}
        assert sorted(row) == sorted(k for k, _ in dacs.model.named_parameters())
        for it in range(iters):
            p = f'{case}.it{it}'
            cj, bl, sigma = [float(v) for v in g[f'{p}.gates']]
            cls = torch.full((1, dacs._kmax()), -1, dtype=torch.int64)
            cls[0, :g[f'{p}.classes'].numel()] = g[f'{p}.classes']
            dacs.inject_draws = dict(choice=float(g[f'{p}.choice']), color_jitter=cj, blur=bl, sigma=sigma, classes=cls, jitter=None,
                                     direction=DIRECT[int(cj * 10) % 2][int(cj * 100) % 2], sky=None, isr_noise=None)
            batch = dict(source={k: v.clone().cuda() for k, v in src.items()}, target={k: v.clone().cuda() for k, v in tg.items()})
            seen = {}
            fwd = dacs.forward_train

            def keep_loss(**kw):   # (train_step drops 'loss' from the log values, dacs.py:304-306: kept here)
                out = fwd(**kw)
                seen['loss'] = out['loss']
                return out
            dacs.forward_train = keep_loss
            try:
                res = dacs.train_step(batch, opt)
            finally:
                del dacs.forward_train
            torch.cuda.synchronize()
            lv = dict(res['log_vars'])
            assert sorted(lv.keys()) == sorted(g[f'{p}.log_keys']), f'{p} log_vars keys'
            lv['loss'] = seen['loss']
            ref = g[f'{p}.losses'].float()
            have = [i for i, k in enumerate(LOSS_KEYS) if k in lv]
            assert [LOSS_KEYS[i] for i in range(7) if not torch.isnan(ref[i])] == [LOSS_KEYS[i] for i in have]
            got = torch.tensor([float(lv.get(k, float('nan'))) for k in LOSS_KEYS])
            print(p, mode, 'losses', got.tolist(), 'reference', ref.tolist())
            tol_l = (1e-4 if exact else 3e-4) * (1 if it == 0 else 10)
            li = [i for i in have if 'acc' not in LOSS_KEYS[i]]
            for i in li:   # each loss against its own reference value
                check_le(f'{p} {LOSS_KEYS[i]} vs reference, rel', abs(got[i] - ref[i]).item() / abs(ref[i]).item(), tol_l)
            ai = [i for i in have if 'acc' in LOSS_KEYS[i]]
            check_le(f'{p} accuracies vs reference (points)', (got[ai] - ref[ai]).abs().max().item(), 0.1 if it == 0 else 0.5)
            mix = dacs.last_mix
            plab = mix['pseudo_label'].cpu().view(1, 512, 512)[..., ::8, ::8].to(torch.uint8)
            check_le(f'{p} pseudo-label disagreement', 1 - (plab.flatten() == g[f'{p}.pseudo_label_s'].flatten()).float().mean().item(),
                     1e-3 if it == 0 else 1e-2)
            mlab = mix['mixed_lbl'].cpu().view(1, 512, 512)[..., ::8, ::8].to(torch.uint8)
            check_le(f'{p} mixed-label disagreement', 1 - (mlab.flatten() == g[f'{p}.mixed_lbl_s'].flatten()).float().mean().item(),
                     1e-3 if it == 0 else 1e-2)
            assert_close(mix['mixed_img'][..., ::16, ::16], g[f'{p}.mixed_img_s'], 1e-6, name=f'{p} mixed image')
            second = mix['mixed_events'] if case == 'events' else mix['mixed_isr']
            assert_close(second.cpu()[:, :1, ::4, ::4], g[f'{p}.mixed_second_s'].float(), 1e-3, name=f'{p} mixed second input')
            none = set(g[f'{case}.grad_none'])
            worst_g = 0.0
            for k, q in dacs.model.named_parameters():
                if k in none:   # what the reference leaves without a gradient gets none here, or zeros
                    assert q.grad is None or not bool(q.grad.abs().sum().item() > 0), f'{k}: gradient where the reference has none'
                    continue
                worst_g = max(worst_g, _fp_rel(sample_grad(q.grad.cpu(), FP_N), g[f'{p}.grad'][row[k]]))
            check_le(f'{p} {mode} worst gradient fingerprint error vs reference', worst_g,
                     (1.2e-2 if exact else 3e-2) if it == 0 else (0.3 if exact else 0.4))
            worst_e = max(_fp_rel(sample_grad(q.detach().cpu(), FP_N), g[f'{p}.ema'][row[k]]) for k, q in dacs.ema_model.named_parameters())
            check_le(f'{p} {mode} worst EMA fingerprint error vs reference', worst_e, 1e-3 if it == 0 else 1e-2)
    finally:
        if dacs is not None:
            dacs.inject_draws = None
        rt.set_gemm_x3(False)
        rt.set_compute_dtype(torch.float32)


@pytest.mark.gpu
def test_dacs_hook_composes_with_the_feature_distance_gpu():
    """enable_fdist on the same route: both terms are logged, and the consistency values equal the run without the feature distance"""
    tgt = _gpu()
    rt.set_compute_dtype(torch.float32)
    plain = small_iteration(tgt, small_dacs(tgt, 'isr'))
    dacs = small_dacs(tgt, 'isr', imnet_feature_dist_lambda=0.005)
    seeded_fill(dacs.imnet_model, 10)
    both = small_iteration(tgt, dacs)
    assert 'src.loss_imnet_feat_dist' in both and np.isfinite(both['src.loss_imnet_feat_dist']) and both['src.loss_imnet_feat_dist'] > 0
    for k in FC_KEYS:   # (the consistency launch is deterministic, and the features do not depend on the feature distance)
        assert both[k] == plain[k], k
    for k in ('decode.loss_seg', 'mix.decode.loss_seg', 'loss'):
        assert_close(torch.tensor([both[k]]), torch.tensor([plain[k]]), 1e-5, name=k)


@pytest.mark.gpu
@pytest.mark.parametrize('lanes', [None, ()])
def test_nofusion_graph_replay_matches_eager_gpu(lanes):
    """three iterations on the ISR route, eager against hipGraph replay (lanes on / off): the same consistency values (device scalars,
    valid after the replay), image-encoder gradients within the bounds of test_fdist.py::test_dacs_fdist_graph_replay_matches_eager_gpu"""
    tgt = _gpu()
    rt.set_compute_dtype(torch.float32)
    src, tg = TD.make_batch(2, 64, 64)
    runs = []
    for graph in (False, True):
        dacs = small_dacs(tgt, 'isr')
        torch.manual_seed(11), random.seed(11), np.random.seed(11)
        if graph:
            dacs.enable_graph(warmup_iters=1)
            if lanes is not None:
                dacs.graph_lane_set = set(lanes)
        batch = dict(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
        out = []
        for it in range(3):
            for p in dacs.model.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            lv = dacs(**batch)
            torch.cuda.synchronize()
            out.append(({k: float(v) for k, v in lv.items() if 'loss' in k},
                        {n: p.grad.detach().cpu().clone() for n, p in dacs.model.named_parameters() if n.startswith('backbone_image.')}))
        if graph:
            assert dacs._graph is not None, 'the iteration was not captured'
        runs.append(out)
    for it, ((l_e, g_e), (l_g, g_g)) in enumerate(zip(*runs)):
        assert l_e.keys() == l_g.keys() and set(FC_KEYS) <= set(l_e) and all(np.isfinite(v) and v > 0 for v in l_e.values())
        for k in l_e:
            assert_close(torch.tensor([l_g[k]]), torch.tensor([l_e[k]]), 1e-4, name=f'it{it} {k}, graph vs eager')
        check_le(f'it{it} replayed loss vs mix loss_seg + loss_feat_consis, rel (two fp32 ulps)',
                 abs(l_g['loss'] - l_g['mix.decode.loss_seg'] - l_g['mix.decode.loss_feat_consis']) / l_g['loss'], 2.0 ** -22)
        worst = max((g_g[n] - q).abs().max().item() / (q.abs().max().item() + 1e-12) for n, q in g_e.items())
        check_le(f'it{it} worst image-encoder gradient rel error, graph vs eager', worst, 5e-2, strict=True)
