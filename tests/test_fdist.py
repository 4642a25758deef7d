"""ImageNet feature distance of DACS (dacs.py:318-354, :566-577; utils/utils.py:18-39): the two kernels of feat_dist.hip against
the reference's downscale_label_ratio (tests/golden/downscale_label.npz) and torch autograd, the frozen ImageNet model's
construction, and the whole step against the reference's own DACS with imnet_feature_dist_lambda = 0.005
(tests/golden/dacs_step_fdist.npz, written by tests/golden/make_golden_fdist.py)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import DACS_CH, DACS_DIMS, DACS_SEEDS, DACS_SEG_SCALE, dacs_batch, sample_grad, seeded_fill  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import ops  # noqa: E402
from cmda_amd._lib import CmdaError  # noqa: E402
from cmda_amd.config import Config, apply_launcher_defaults  # noqa: E402
from cmda_amd.registry import build_train_model  # noqa: E402
from conftest import assert_close, check_le  # noqa: E402

FD_CLASSES = [6, 7, 11, 12, 13, 14, 15, 16, 17, 18]
FD_SEED_IMNET = 114
SMALL = dict(dims=[32, 64, 160, 256], ch=64)
ISR = dict(val_range=[0.01, 1.01], _threshold=0.005, _clip_range=0.1, shift_pixel=1)
FCFG = dict(loss_weight={'image': 0.5, 'events': 0.5, 'fusion': 0.5, 'img_self_res': 0.25}, gradual_rate=0.0)


def golden(name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', name)).items()}


def make_cfg(dims, ch, lam=0.005, classes=FD_CLASSES, ratio=0.75):
    """the reduced-width fusion DACS of tests/test_dacs.py (generator on, reference draws) with the feature distance switched on"""
    bb = dict(type='MixVisionTransformer', embed_dims=dims, num_heads=[1, 2, 5, 8], qkv_bias=True, depths=[1, 1, 1, 1],
              sr_ratios=[8, 4, 2, 1], drop_path_rate=0.0, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6))
    head = dict(type='DAFormerHeadFusion', in_channels=dims, in_index=[0, 1, 2, 3], channels=ch, dropout_ratio=0.0, num_classes=19,
                norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
                decoder_params=dict(embed_dims=ch, embed_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                                    embed_neck_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                                    fusion_cfg=dict(type='aspp', sep=True, dilations=(1, 6, 12, 18), pool=False,
                                                    act_cfg=dict(type='ReLU'), norm_cfg=dict(type='BN', requires_grad=True)),
                                    train_type='cs2dsec_image+events_together', share_decoder=True),
                loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    model = dict(type='FusionEncoderDecoder', backbone_image=dict(bb), backbone_events=dict(bb),
                 fusion_module=dict(type='AttentionAvgFusion', in_channels=dims, drop_path_rate=0.0), decode_head=head,
                 train_type='cs2dsec_image+events_together', train_cfg=dict(), test_cfg=dict(mode='whole'))
    uda = dict(type='DACS', alpha=0.999, pseudo_threshold=0.968, pseudo_weight_ignore_top=0, pseudo_weight_ignore_bottom=0,
               imnet_feature_dist_lambda=lam, imnet_feature_dist_classes=classes, imnet_feature_dist_scale_min_ratio=ratio,
               mix='class', blur=True, color_jitter_strength=0.2, color_jitter_probability=0.2, debug_img_interval=1000,
               print_grad_magnitude=False, train_type='cs2dsec_image+events_together', forward_cfg=dict(FCFG),
               cyclegan_itrd2en_path='random', img_self_res_reg='no', mixed_image_to_mixed_isr=True, random_choice_thres='0.5',
               shift_type='random', isr_parms=dict(ISR), sky_mask=None)
    return dict(model=model, uda=uda, runner=dict(type='IterBasedRunner', max_iters=40000))


# ---------------------------------------------------------------------------------------------------------------------------
# kernels (emulator build of the same sources, and the GPU)
def test_fdist_label_mask_matches_reference(tgt):
    g = golden('downscale_label.npz')
    for s in (2, 4, 8, 32):
        lab = g[f's{s}.label'].long()
        lab[lab == 255] = 255
        B, _, H, W = lab.shape
        for r in (75, 50, 25):
            resc, mask, count = ops.fdist_label_mask(tgt.to(lab.view(B, H, W).contiguous()), H // s, W // s, FD_CLASSES, r / 100)
            ref_r = g[f's{s}.r{r}.rescaled'].long().view(B, H // s, W // s)
            ref_m = g[f's{s}.r{r}.mask'].view(B, H // s, W // s)
            assert torch.equal(resc.cpu(), ref_r), f's={s} min_ratio={r / 100}: rescaled label differs'
            assert torch.equal(mask.cpu().bool(), ref_m), f's={s} min_ratio={r / 100}: mask differs'
            assert int(count.cpu()) == int(ref_m.sum()), f's={s} min_ratio={r / 100}: count {int(count.cpu())} vs {int(ref_m.sum())}'
    # H, W not multiples of the cell size: an error, not a launch
    with pytest.raises(CmdaError):
        ops.fdist_label_mask(tgt.to(torch.zeros(1, 65, 64, dtype=torch.int64)), 2, 2, FD_CLASSES, 0.75)


def _autograd(fs, ft, lam, mask):
    x = fs.detach().float().requires_grad_(True)
    d = torch.norm(x - ft.float(), dim=1, p=2)
    if mask is not None:
        d = d[mask.bool()]
    loss = lam * torch.mean(d)
    if mask is None or mask.any():
        loss.backward()
        return loss.detach(), x.grad
    return loss.detach(), torch.zeros_like(x)


@pytest.mark.parametrize('case', ['mask', 'no_mask', 'empty_mask', 'zero_rows', 'accumulate', 'bf16', 'bf16_f32_grad'])
def test_fdist_distance_matches_autograd(tgt, case):
    g = torch.Generator().manual_seed(5)
    R, C = 2 * 4 * 4, 256
    dt = torch.bfloat16 if case.startswith('bf16') else torch.float32
    fs = torch.randn(R, C, generator=g).to(dt)
    ft = torch.randn(R, C, generator=g).to(dt)
    mask = (torch.rand(R, generator=g) < 0.5).to(torch.uint8)
    if case == 'no_mask':
        mask = None
    elif case == 'empty_mask':
        mask.zero_()
    elif case == 'zero_rows':
        ft[::3] = fs[::3]
        mask[::3] = 1
    gdt = torch.float32 if case == 'bf16_f32_grad' else dt
    # a non-zero block of the FD gradient's own magnitude (~lambda / count / sqrt(C)): the added part stays visible in fp32
    grad0 = (1e-4 * torch.randn(R, C, generator=g) if case in ('accumulate', 'bf16', 'bf16_f32_grad') else torch.zeros(R, C)).to(gdt)
    gscale = 0.5 if case in ('accumulate', 'bf16', 'bf16_f32_grad') else 1.0
    lam = 0.005
    count = None if mask is None else mask.sum().to(torch.int32).view(1)
    grad = tgt.to(grad0.clone())
    loss, norms = ops.fdist_fwd_bwd(tgt.to(fs), tgt.to(ft), lam, mask=tgt.to(mask), count=tgt.to(count),
                                    gscale=tgt.to(torch.tensor([gscale])), grad=grad)
    ref_loss, ref_grad = _autograd(fs, ft, lam, mask)
    loss, grad = loss.cpu(), grad.cpu()
    if case == 'empty_mask':
        assert torch.isnan(loss).all(), 'an empty mask must give a NaN loss (torch.mean of nothing)'
        assert torch.equal(grad, grad0), 'an empty mask must leave the gradient untouched'
        return
    expect = grad0.float() + gscale * ref_grad
    if dt == torch.float32:
        assert_close(loss, ref_loss.view(1), 1e-5, name=f'{case} loss')
        assert_close(grad - grad0, gscale * ref_grad, 1e-5, name=f'{case} added gradient')
    else:
        check_le(f'{case} loss rel err', (loss - ref_loss).abs().item() / ref_loss.abs().item(), 1e-5)
        # bf16 gradient block: the sum is rounded once to bf16 (2^-8 relative); fp32 block: fp32 round-off of the sum
        tol = 2 * 2 ** -8 if gdt == torch.bfloat16 else 2e-5   # (measured 3.9e-3 / 9.1e-6)
        err = ((grad.float() - expect).abs() / expect.abs().clamp_min(1e-30)).max().item()
        check_le(f'{case} gradient rel err (elementwise)', err, tol)
    if case == 'zero_rows':
        assert (grad[::3] == 0).all(), 'a zero-difference row contributes gradient 0 (torch.norm backward), not NaN'
        assert torch.isfinite(grad).all()


# ---------------------------------------------------------------------------------------------------------------------------
# construction (CPU)
def test_dacs_fdist_state_dict_keys_match_reference():
    with torch.device('meta'):
        dacs = build_train_model(make_cfg(DACS_DIMS, DACS_CH))
    with open(os.path.join(HERE, 'golden', 'dacs_fdist_keys.json')) as f:
        ref = json.load(f)
    # (as tests/test_registry_config.py: the key SET and shapes' names; the module registration order inside MiT differs)
    assert sorted(dacs.state_dict().keys()) == sorted(ref)
    assert sum(k.startswith('imnet_model.') for k in ref) > 0


def test_dacs_fdist_imnet_model_is_frozen_and_outside_the_update():
    from cmda_amd.optim import FlatAdamW
    dacs = build_train_model(make_cfg(SMALL['dims'], SMALL['ch']))
    imnet = list(dacs.imnet_model.parameters())
    assert imnet and all(not p.requires_grad and getattr(p, '_cmda_frozen', False) for p in imnet)
    ids = {id(p) for p in imnet}
    opt = FlatAdamW(dacs.model)
    flat = opt.flat_p
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size()
    assert not any(lo <= p.data_ptr() < hi for p in imnet), 'an ImageNet-model weight lives in the optimizer store'
    assert not ids & {id(p) for p in dacs.model.parameters()}
    assert not ids & {id(p) for p in dacs.ema_model.parameters()}, 'an ImageNet-model weight is an EMA pair'
    # the data-parallel reducer buckets FlatAdamW's flat gradient: it holds exactly the optimizer's parameters
    n_store = sum(p.numel() for p in dacs.model.parameters() if p.requires_grad)
    assert opt.flat_p.numel() >= n_store and all(p.grad is None for p in imnet)
    # lambda = 0: nothing is built
    assert build_train_model(make_cfg(SMALL['dims'], SMALL['ch'], lam=0)).imnet_model is None


@pytest.mark.parametrize('name', ['cs2dsec_image+events_together_b5', 'cs2dz_image+raw-isr_b5'])
def test_fusion_configs_build_with_fdist(name):
    cfg = Config.fromfile(os.path.join(HERE, 'golden', 'configs', name + '.json'))
    cfg = apply_launcher_defaults(cfg, feature_dist=0.005)
    assert cfg.uda.imnet_feature_dist_lambda == 0.005
    cfg.model.pretrained = None
    cfg.uda.cyclegan_itrd2en_path = 'random' if cfg.uda.get('cyclegan_itrd2en_path') else ''
    with torch.device('meta'):
        dacs = build_train_model(cfg)
    assert dacs.imnet_model is not None and dacs.fdist_classes == FD_CLASSES and dacs.fdist_scale_min_ratio == 0.75
    keys = dacs.state_dict().keys()
    assert any(k.startswith('imnet_model.backbone.') for k in keys) and any(k.startswith('imnet_model.decode_head.') for k in keys)
    assert all(not p.requires_grad for p in dacs.imnet_model.parameters())
    assert apply_launcher_defaults(Config.fromfile(os.path.join(HERE, 'golden', 'configs', name + '.json'))).uda.imnet_feature_dist_lambda == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the step on the GPU
def _gpu():
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    return Target('gpu')


def _fixture_dacs(lam, route):
    dacs = build_train_model(make_cfg(DACS_DIMS, DACS_CH, lam=lam))
    seeded_fill(dacs.model, DACS_SEEDS['student'])
    seeded_fill(dacs.ema_model, DACS_SEEDS['teacher'])
    seeded_fill(dacs.cyclegan_itrd2en, DACS_SEEDS['generator'])
    if dacs.imnet_model is not None:
        seeded_fill(dacs.imnet_model, FD_SEED_IMNET)
    with torch.no_grad():
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    if route == 'two_pass':
        dacs.fused_student_passes = False
        dacs.model.joint_passes = False
    return dacs.to('cuda:0').train()


def _fixture_step(dacs, opt, g, src, tg, it):
    cj, bl, sigma = [float(v) for v in g[f'it{it}.gates']]
    cls = torch.full((1, dacs._kmax()), -1, dtype=torch.int64)
    cls[0, :g[f'it{it}.classes'].numel()] = g[f'it{it}.classes']
    dacs.inject_draws = dict(choice=float(g[f'it{it}.choice']), color_jitter=cj, blur=bl, sigma=sigma, classes=cls, jitter=None,
                             direction=[['leftdown', 'leftup'], ['rightdown', 'rightup']][int(cj * 10) % 2][int(cj * 100) % 2])
    batch = dict(source={k: v.clone().cuda() for k, v in src.items()}, target={k: v.clone().cuda() for k, v in tg.items()})
    res = dacs.train_step(batch, opt)
    torch.cuda.synchronize()
    return res


def _fp_rel(got, ref):
    """fingerprint error as in test_dacs: sample relative to its largest element, sums relative to the abs-sum"""
    return max((got[:-2] - ref[:-2]).abs().max().item() / (ref[:-2].abs().max().item() + 1e-12),
               (got[-2:] - ref[-2:]).abs().max().item() / (ref[-1].abs().item() + 1e-12))


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['fused', 'two_pass'])
@pytest.mark.parametrize('mode', ['f32', 'x3'])
def test_dacs_fdist_step_against_reference_fixture_gpu(mode, route):
    from cmda_amd.optim import FlatAdamW
    _gpu()
    g = golden('dacs_step_fdist.npz')
    src, tg = dacs_batch()
    src['label'] = g['label'].long()
    exact = mode == 'f32'
    rt.set_compute_dtype(torch.float32)
    rt.set_gemm_x3(mode == 'x3')
    dacs = None
    try:
        # the FD gradient in isolation: iteration 0 with lambda = 0.5 minus lambda = 0, image encoder, against the reference's
        grads = {}
        for tag, lam in (('lam0', 0.0), ('lam05', 0.5)):
            dacs = _fixture_dacs(lam, route)
            opt = FlatAdamW(dacs.model, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
            _fixture_step(dacs, opt, g, src, tg, 0)
            grads[tag] = {k: sample_grad(p.grad.cpu(), 24) for k, p in dacs.model.named_parameters() if k.startswith('backbone_image.')}
            dacs.inject_draws = None
        worst = 0.0
        for k in grads['lam0']:
            got = (grads['lam05'][k] - grads['lam0'][k])[:-1]   # sample + sum (the abs-sum is not linear)
            ref = (g[f'lam05.grad.{k}'] - g[f'lam0.grad.{k}'])[:-1]
            worst = max(worst, (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12))
        # measured on MI355X: f32 7.8e-3 / 3.0e-3, split-bf16 1.15e-2 / 2.4e-2 (fused / two-pass route); 2x headroom
        check_le('FD gradient (lambda 0.5 - 0) of the image encoder vs reference, rel', worst, 1.6e-2 if exact else 5e-2)

        dacs = _fixture_dacs(0.005, route)
        opt = FlatAdamW(dacs.model, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
        imnet0 = {k: p.detach().cpu().clone() for k, p in dacs.imnet_model.named_parameters()}
        for it in range(2):
            res = _fixture_step(dacs, opt, g, src, tg, it)
            lv = res['log_vars']
            ref_l = g[f'it{it}.losses'].float()
            got = torch.tensor([float(lv['decode.loss_seg']), float(lv['mix.decode.loss_seg']), float(lv['src.loss_imnet_feat_dist'])])
            tol_l = (1e-4 if exact else 3e-4) * (1 if it == 0 else 10)
            assert_close(got, ref_l[[0, 2, 4]], tol_l, name=f'it{it} losses (source, mixed, feature distance) vs reference')
            assert torch.equal(dacs.debug_fdist_mask.cpu(), g[f'it{it}.fdist_mask']), f'it{it} feature-distance mask'
            assert torch.equal(dacs.debug_gt_rescale.cpu().to(torch.uint8), g[f'it{it}.gt_rescale']), f'it{it} rescaled label'
            worst = 0.0
            for k, p in dacs.model.named_parameters():
                worst = max(worst, _fp_rel(sample_grad(p.grad.cpu(), 24), g[f'it{it}.grad.{k}']))
            # the bounds of test_dacs.py::test_dacs_train_step_against_reference_fixture_gpu
            check_le(f'it{it} worst gradient fingerprint error vs reference', worst,
                     (1.2e-2 if exact else 3e-2) if it == 0 else (0.3 if exact else 0.4))
        for k, p in dacs.imnet_model.named_parameters():
            assert torch.equal(p.detach().cpu(), imnet0[k]), f'imnet_model.{k} changed'
            assert p.grad is None
    finally:
        if dacs is not None:
            dacs.inject_draws = None
        rt.set_gemm_x3(False)
        rt.set_compute_dtype(torch.float32)


def _cell_label(B, H, W):
    """32 x 32 cells: FD classes at full and at 3/4 ratio, other classes, a mixed cell -- a mask that is neither empty nor full"""
    lab = torch.zeros(B, 1, H, W, dtype=torch.int64)
    vals = [6, 2, 12, 255, 17, 0, 13, 7]
    for b in range(B):
        for i in range(H // 32):
            for j in range(W // 32):
                v = vals[(b * 3 + i * (W // 32) + j) % len(vals)]
                lab[b, 0, i * 32:(i + 1) * 32, j * 32:(j + 1) * 32] = v
                if v == 12:
                    lab[b, 0, i * 32:i * 32 + 8, j * 32:(j + 1) * 32] = 1     # 3/4 of the cell: still in the mask
                if v == 0:
                    lab[b, 0, i * 32:i * 32 + 16, j * 32:(j + 1) * 32] = 15   # tie below the ratio: out
    return lab


@pytest.mark.gpu
@pytest.mark.parametrize('lanes', [None, ()])
def test_dacs_fdist_graph_replay_matches_eager_gpu(lanes):
    """three iterations with the feature distance on, eager against hipGraph replay (lanes on / off): same FD loss, image-encoder
    gradients within the bounds of test_dacs_graph_replay_matches_oracle"""
    import random
    tgt = _gpu()
    sys.path.insert(0, HERE)
    from test_dacs import make_batch
    rt.set_compute_dtype(torch.float32)
    src, tg = make_batch(2, 64, 64)
    src['label'] = _cell_label(2, 64, 64)
    runs = []
    for graph in (False, True):
        dacs = build_train_model(make_cfg(SMALL['dims'], SMALL['ch']))
        seeded_fill(dacs.model, 7)
        seeded_fill(dacs.ema_model, 8)
        seeded_fill(dacs.cyclegan_itrd2en, 9)
        seeded_fill(dacs.imnet_model, 10)
        dacs.to(tgt.device).train()
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
            out.append((float(lv['src.loss_imnet_feat_dist']), dacs.debug_fdist_mask.cpu().clone(),
                        {n: p.grad.detach().cpu().clone() for n, p in dacs.model.named_parameters() if n.startswith('backbone_image.')}))
        if graph:
            assert dacs._graph is not None, 'the iteration was not captured'
        runs.append(out)
    for it, ((l_e, m_e, g_e), (l_g, m_g, g_g)) in enumerate(zip(*runs)):
        assert np.isfinite(l_e) and 0 < int(m_e.sum()) < m_e.numel()
        assert torch.equal(m_e, m_g)
        assert_close(torch.tensor([l_g]), torch.tensor([l_e]), 1e-4, name=f'it{it} feature-distance loss, graph vs eager')
        worst = max((g_g[n] - q).abs().max().item() / (q.abs().max().item() + 1e-12) for n, q in g_e.items())
        check_le(f'it{it} worst image-encoder gradient rel error, graph vs eager', worst, 5e-2, strict=True)


@pytest.mark.gpu
def test_dacs_fdist_full_size_bf16_graph_gpu():
    """MiT-B5 at 512 x 512, bf16, graph replay, feature distance on, one replayed iteration: the FD loss is finite and agrees with a
    torch recompute from the step's own stage-4 features and mask; the decode losses equal a lambda = 0 run's"""
    import random
    tgt = _gpu()
    B, H, W = 2, 512, 512
    g = torch.Generator().manual_seed(21)
    src = dict(image=torch.randn(B, 3, H, W, generator=g), img_time_res=torch.rand(B, 3, H, W, generator=g) * 2 - 1,
               img_self_res=torch.rand(B, 3, H, W, generator=g) * 2 - 1, label=_cell_label(B, H, W))
    tg = dict(warp_image=torch.randn(B, 3, H, W, generator=g), events_vg=torch.rand(B, 3, H, W, generator=g) * 2 - 1,
              warp_img_self_res=torch.rand(B, 3, H, W, generator=g) * 2 - 1)
    dims = [64, 128, 320, 512]
    rt.set_compute_dtype(torch.bfloat16)
    res = {}
    try:
        for lam in (0.005, 0.0):
            cfg = make_cfg(dims, 256, lam=lam)
            for k in ('backbone_image', 'backbone_events'):
                cfg['model'][k].update(depths=[3, 6, 40, 3], drop_path_rate=0.0)
            dacs = build_train_model(cfg)
            seeded_fill(dacs.model, 7)
            seeded_fill(dacs.ema_model, 8)
            seeded_fill(dacs.cyclegan_itrd2en, 9)
            if dacs.imnet_model is not None:
                seeded_fill(dacs.imnet_model, 10)
            dacs.to(tgt.device).train()
            dacs.enable_graph(warmup_iters=1)
            batch = dict(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
            for it in range(2):
                torch.manual_seed(11 + it), random.seed(11 + it), np.random.seed(11 + it)
                for p in dacs.model.parameters():
                    if p.grad is not None:
                        p.grad.zero_()
                lv = dacs(**batch)
            torch.cuda.synchronize()
            assert dacs._graph is not None
            out = {k: float(v) for k, v in lv.items() if 'loss' in k}
            if lam > 0:
                mix = dacs.last_mix
                ft = mix['fdist_feat_imnet'].float()
                # the student's stage-4 features of the source rows: recomputed by its own image encoder (eval of the same weights)
                with torch.no_grad():
                    feats, _ = dacs.model.backbone_image.fwd(batch['source']['image'], save=False)
                fs = feats[3][0].float()
                m = dacs.debug_fdist_mask.view(-1)
                ref = lam * torch.norm(fs - ft, dim=1)[m].mean().item()
                out['recompute'] = ref
                out['mask'] = int(m.sum())
            res[lam] = out
            del dacs
            torch.cuda.empty_cache()
    finally:
        rt.set_compute_dtype(torch.float32)
    on, off = res[0.005], res[0.0]
    print('FD on', on, 'FD off', off)
    assert np.isfinite(on['src.loss_imnet_feat_dist']) and 0 < on['mask'] < 2 * 16 * 16
    check_le('FD loss vs torch recompute, rel', abs(on['src.loss_imnet_feat_dist'] - on['recompute']) / abs(on['recompute']), 1e-2)
    for k in ('decode.loss_seg', 'mix.decode.loss_seg'):
        check_le(f'{k}: FD on vs off, rel', abs(on[k] - off[k]) / abs(off[k]), 2e-2)
