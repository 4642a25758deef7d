"""Image-only DACS train types 'cs2dsec_image' / 'cs2dz_image' (dacs.py:83-85, :363-377, the image branches of forward_train;
EventsEncoderDecoder encoder_decoder.py:308-620): construction and state-dict keys, the rejected forms, the host draws, the
three-output-channel stencil of the day -> night generator (conv_co1.hip, cmda_conv_co3) against torch on the emulator and the GPU,
the 3 -> 3 generator, simple_test and the whole step against the reference's own code (tests/golden/dacs_step_image.npz,
generator_33.npz, image_simple_test.npz, dacs_image_keys.json, written by tests/golden/make_golden_image.py), graph replay against
eager, the gradient-ready hook, and a full-depth MiT-B5 bf16 step."""
import functools
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import DACS_CH, DACS_DIMS, DACS_SEG_SCALE, dacs_batch, sample_grad, seeded_fill, seeded_randn  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import ops  # noqa: E402
from cmda_amd._lib import CmdaError  # noqa: E402
from cmda_amd.registry import build_segmentor, build_train_model  # noqa: E402
from conftest import assert_close, check_le  # noqa: E402

FD_CLASSES = [6, 7, 11, 12, 13, 14, 15, 16, 17, 18]
SEEDS = dict(student=121, teacher=122, imnet=124, generator=123, label=125, g33=131, simple=141)
FP_N = 16   # samples per fingerprint in dacs_step_image.npz
MEAN, STD = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])


def golden(name):
    """numeric arrays as tensors, string arrays (the log keys) as lists"""
    return {k: (v.tolist() if v.dtype.kind == 'U' else torch.from_numpy(v)) for k, v in np.load(os.path.join(HERE, 'golden', name)).items()}


def model_cfg(dims, ch, depths=(1, 1, 1, 1)):
    bb = dict(type='MixVisionTransformer', embed_dims=dims, num_heads=[1, 2, 5, 8], qkv_bias=True, depths=list(depths),
              sr_ratios=[8, 4, 2, 1], drop_path_rate=0.0, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6))
    head = dict(type='DAFormerHead', in_channels=dims, in_index=[0, 1, 2, 3], channels=ch, dropout_ratio=0.0, num_classes=19,
                norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
                decoder_params=dict(embed_dims=ch, embed_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                                    embed_neck_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                                    fusion_cfg=dict(type='aspp', sep=True, dilations=(1, 6, 12, 18), pool=False,
                                                    act_cfg=dict(type='ReLU'), norm_cfg=dict(type='BN', requires_grad=True))),
                loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    return dict(type='EventsEncoderDecoder', backbone=bb, decode_head=head, train_cfg=dict(), test_cfg=dict(mode='whole'))


def make_cfg(train_type, dims=DACS_DIMS, ch=DACS_CH, lam=0.0, generator=False, depths=(1, 1, 1, 1), **extra):
    """the reference's image-only DACS at reduced width (make_golden_image.image_cfg)"""
    uda = dict(type='DACS', alpha=0.999, pseudo_threshold=0.968, pseudo_weight_ignore_top=0, pseudo_weight_ignore_bottom=0,
               imnet_feature_dist_lambda=lam, imnet_feature_dist_classes=list(FD_CLASSES), imnet_feature_dist_scale_min_ratio=0.75,
               mix='class', blur=True, color_jitter_strength=0.2, color_jitter_probability=0.2, debug_img_interval=1000,
               print_grad_magnitude=False, train_type=train_type, forward_cfg=dict(), img_self_res_reg='no', sky_mask=None,
               cyclegan_id2in_path='random' if generator else '', **extra)
    return dict(model=model_cfg(dims, ch, depths), uda=uda, runner=dict(type='IterBasedRunner', max_iters=40000))


def image_batch(train_type, g):
    """make_golden_image.image_batch: dacs_batch's source image, the fixture's cell-aligned label, the target image under the type's key"""
    src, tg = dacs_batch()
    src = dict(image=src['image'], label=g['label'].long())
    tg = dict(warp_image=tg['warp_image']) if train_type == 'cs2dsec_image' else dict(image=tg['warp_image'])
    return src, tg


# ---------------------------------------------------------------------------------------------------------------------------
# construction (no GPU)
def test_image_types_build_with_reference_keys():
    ref = json.load(open(os.path.join(HERE, 'golden', 'dacs_image_keys.json')))
    with torch.device('meta'):
        dacs = build_train_model(make_cfg('cs2dsec_image', lam=0.005))
    assert type(dacs.model).__name__ == 'EventsEncoderDecoder' and type(dacs.imnet_model).__name__ == 'EventsEncoderDecoder'
    assert sorted(dacs.state_dict().keys()) == sorted(ref)
    assert all(not p.requires_grad for p in dacs.imnet_model.parameters())
    with torch.device('meta'):
        dz = build_train_model(make_cfg('cs2dz_image', generator=True))
    gen = [k for k in dz.state_dict() if k.startswith('cyclegan_id2in.')]
    assert sorted(k for k in dz.state_dict() if not k.startswith('cyclegan_id2in.')) == sorted(k for k in ref if not k.startswith('imnet_model.'))
    assert gen and dz.cyclegan_id2in.model[1].in_channels == 3 and dz.cyclegan_id2in.model[-2].out_channels == 3
    assert all(not p.requires_grad for p in dz.cyclegan_id2in.parameters())
    # the DSEC type has no generator (dacs.py:105: 'cs2dz_image' only)
    with torch.device('meta'):
        assert build_train_model(make_cfg('cs2dsec_image', generator=True)).cyclegan_id2in is None


def test_image_types_reject_out_of_scope_forms():
    with pytest.raises(ValueError, match='LightNet'):
        with torch.device('meta'):
            build_train_model(make_cfg('cs2dz_image', cyclegan_light_path='light.pth'))
    cfg = model_cfg(DACS_DIMS, DACS_CH)
    cfg['backbone']['in_chans'] = 6
    with pytest.raises(ValueError, match='image-only'):
        with torch.device('meta'):
            build_segmentor(cfg)
    with torch.device('meta'):
        m = build_segmentor(model_cfg(DACS_DIMS, DACS_CH))
    x = torch.zeros(1, 3, 64, 64)
    for call in (lambda: m.forward_train(x, x, torch.zeros(1, 1, 64, 64, dtype=torch.long)), lambda: m.encode_decode(x, x),
                 lambda: m.extract_feat(x, x), lambda: m.encode_decode_lowres(None, x)):
        with pytest.raises((NotImplementedError, ValueError)):
            call()


def test_image_draw_consumes_no_choice():
    """dacs.py:446-456 then get_class_masks: three random.uniform draws, the class draw -- and no torch.rand (the events / ISR choice
    of :414-417 exists only in the events branch)"""
    with torch.device('meta'):
        dacs = build_train_model(make_cfg('cs2dsec_image'))
    lab = torch.randint(0, 19, (2, 1, 16, 16), generator=torch.Generator().manual_seed(0))
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    d = dacs._draw(lab, 16, 16)
    after_py, after_np, after_t = random.random(), np.random.get_state()[1][:4].copy(), torch.rand(1)
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    cj, bl, sg = random.uniform(0, 1), random.uniform(0, 1), random.uniform(0.15, 1.15)
    classes = torch.unique(lab)
    n = classes.shape[0]
    picks = [np.random.choice(n, int((n + n % 2) / 2), replace=False) for _ in range(2)]
    jitter = cj > 0.2
    if jitter:   # kornia ColorJitter's per-sample draws (one call per sample) follow, as in the fusion types
        for _ in range(2):
            np.random.permutation(4)
            [random.uniform(0.8, 1.2) for _ in range(3)] + [random.uniform(-0.2, 0.2)]
    assert d['choice'] is None and (d['color_jitter'], d['blur'], d['sigma']) == (cj, bl, sg)
    for i in range(2):
        assert d['classes'][i, :len(picks[i])].tolist() == classes[torch.as_tensor(picks[i])].tolist()
    assert random.random() == after_py and (np.random.get_state()[1][:4] == after_np).all()
    assert torch.equal(torch.rand(1), after_t), 'torch RNG consumed by the image-only draw'


# ---------------------------------------------------------------------------------------------------------------------------
# the three-output-channel stencil (emulator build of the same sources, and the GPU)
@pytest.mark.parametrize('dt,tol', [(torch.bfloat16, 2e-3), (torch.float32, 2e-5)])
def test_conv_co3(tgt, dt, tol):
    """ReflectionPad2d(3) + Conv2d(64, 3, 7) + Tanh, then the per-channel output map, NCHW out (and zero padding, no map)"""
    torch.manual_seed(3)
    B, H, W, C, K = 2, 19, 37, 64, 7
    x = torch.randn(B, C, H, W).to(dt)
    w = (torch.randn(3, C, K, K) * 0.05).to(dt)
    bias = torch.randn(3)
    scale, shift = 0.5 / STD, (0.5 - MEAN) / STD
    xd = tgt.to(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous())
    wd = tgt.to(w.permute(0, 2, 3, 1).reshape(3, -1).contiguous())
    for reflect, affine in ((True, True), (False, False), (True, False)):
        xp = F.pad(x.float(), (3, 3, 3, 3), mode='reflect') if reflect else F.pad(x.float(), (3, 3, 3, 3))
        ref = torch.tanh(F.conv2d(xp, w.float(), bias))
        if affine:
            ref = ref * scale.view(1, 3, 1, 1) + shift.view(1, 3, 1, 1)
        assert ops.conv_co1_ok(xd, C, K, 3)
        out = ops.conv_co3(xd, wd, tgt.to(bias), B, H, W, C, K, 3, reflect, 'tanh',
                           tgt.to(scale) if affine else None, tgt.to(shift) if affine else None)
        assert out.shape == (B, 3, H, W)
        assert_close(out, ref, tol * (4 if affine else 1), name=f'conv_co3 reflect={reflect} affine={affine}')
    with pytest.raises(CmdaError):
        ops.conv_co3(xd, wd, tgt.to(bias), B, H, W, C, K, 3, True, 'tanh', tgt.to(scale), None)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
def _gpu():
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    return Target('gpu')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_generator_33_against_reference_gpu(dtype):
    """define_G(input_nc=3, output_nc=3) -- the first layer with Ci = 3 (channel-padded to 8 in bf16), the last through cmda_conv_co3 --
    against the reference generator; and the input / output maps of set_io_affine against the reference's explicit arithmetic"""
    from cmda_amd.cyclegan import define_G
    _gpu()
    g = golden('generator_33.npz')
    rt.set_compute_dtype(torch.float32 if dtype == 'f32' else torch.bfloat16)
    try:
        G = define_G(input_nc=3, output_nc=3)
        seeded_fill(G, SEEDS['g33'])
        G = G.cuda().eval()
        x = seeded_randn((2, 3, 40, 56), SEEDS['g33'], 'x').cuda()
        y = G(x)
        # (bf16: 23 conv + InstanceNorm layers on random weights, the bound of test_modules.py::test_generator_golden; 4.6e-2 measured)
        assert_close(y, g['y'], 1e-4 if dtype == 'f32' else 0.1, name=f'generator 3->3 {dtype}')
        ygemm = G(x, last_route='gemm')
        assert_close(y, ygemm, 1e-4 if dtype == 'f32' else 1e-2, name=f'stencil vs GEMM last layer {dtype}')
        # dacs.py:369-372: G((x * std + mean - 0.5) / 0.5) / 2 + 0.5 - mean) / std, the maps folded into the generator
        m, s = MEAN.view(1, 3, 1, 1).cuda(), STD.view(1, 3, 1, 1).cuda()
        ref = (G((x * s + m - 0.5) / 0.5) / 2 + 0.5 - m) / s
        G.set_io_affine(2.0 * STD, 2.0 * (MEAN - 0.5), 0.5 / STD, (0.5 - MEAN) / STD)
        assert_close(G(x), ref, 1e-4 if dtype == 'f32' else 0.1, name=f'generator with the io maps {dtype}')
    finally:
        rt.set_compute_dtype(torch.float32)


@pytest.mark.gpu
def test_simple_test_against_reference_gpu():
    _gpu()
    g = golden('image_simple_test.npz')
    rt.set_compute_dtype(torch.float32)
    m = build_segmentor(model_cfg(DACS_DIMS, DACS_CH))
    seeded_fill(m, SEEDS['simple'])
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    m = m.cuda().eval()
    img = seeded_randn((1, 3, 440, 640), SEEDS['simple'], 'img').cuda()
    assert_close(m.encode_decode(img, None)[..., ::16, ::16], g['logit_s'], 1e-4, name='encode_decode logits')
    for key in ('image', 'warp_image'):
        for flip in (False, True):
            meta = dict(ori_shape=(440, 640, 3), flip=flip, flip_direction='horizontal')
            seg = np.stack(m.simple_test(True, **{key: img, 'img_metas': meta}))
            assert seg.shape == (1, 440, 640)
            seg = seg[..., ::4, ::4]   # (the fixture keeps every fourth row / column)
            ref = g[f'{key}.flip{int(flip)}'].numpy()
            agree = (seg == ref).mean()
            check_le(f'simple_test {key} flip={flip}: label disagreement', 1 - agree, 1e-3)


def _fixture_dacs(train_type, lam, generator):
    dacs = build_train_model(make_cfg(train_type, lam=lam, generator=generator))
    seeded_fill(dacs.model, SEEDS['student'])
    seeded_fill(dacs.ema_model, SEEDS['teacher'])
    if dacs.cyclegan_id2in is not None:
        seeded_fill(dacs.cyclegan_id2in, SEEDS['generator'])
    if dacs.imnet_model is not None:
        seeded_fill(dacs.imnet_model, SEEDS['imnet'])
    with torch.no_grad():
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    return dacs.to('cuda:0').train()


def _fixture_step(dacs, opt, g, p, src, tg):
    cj, bl, sigma = [float(v) for v in g[f'{p}.gates']]
    cls = torch.full((1, dacs._kmax()), -1, dtype=torch.int64)
    cls[0, :g[f'{p}.classes'].numel()] = g[f'{p}.classes']
    dacs.inject_draws = dict(choice=None, color_jitter=cj, blur=bl, sigma=sigma, classes=cls, jitter=None, direction='rightdown')
    batch = dict(source={k: v.clone().cuda() for k, v in src.items()}, target={k: v.clone().cuda() for k, v in tg.items()})
    res = dacs.train_step(batch, opt)
    torch.cuda.synchronize()
    return res


def _fp_rel(got, ref):
    return max((got[:-2] - ref[:-2]).abs().max().item() / (ref[:-2].abs().max().item() + 1e-12),
               (got[-2:] - ref[-2:]).abs().max().item() / (ref[-1].abs().item() + 1e-12))


STEP_CASES = [('dsec', 'cs2dsec_image', 0.0, False, 3), ('dsec_fd', 'cs2dsec_image', 0.005, False, 3), ('dz', 'cs2dz_image', 0.0, True, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', [c[0] for c in STEP_CASES])
@pytest.mark.parametrize('mode', ['f32', 'x3'])
def test_image_step_against_reference_fixture_gpu(mode, case):
    from cmda_amd.optim import FlatAdamW
    _gpu()
    tag, tt, lam, gen, iters = [c for c in STEP_CASES if c[0] == case][0]
    g = golden('dacs_step_image.npz')
    src, tg = image_batch(tt, g)
    exact = mode == 'f32'
    rt.set_compute_dtype(torch.float32)
    rt.set_gemm_x3(mode == 'x3')
    dacs = None
    try:
        dacs = _fixture_dacs(tt, lam, gen)
        opt = FlatAdamW(dacs.model, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
        for it in range(iters):
            p = f'{tag}.it{it}'
            res = _fixture_step(dacs, opt, g, p, src, tg)
            lv = res['log_vars']
            assert sorted(lv.keys()) == sorted(g[f'{p}.log_keys']), f'{p} log_vars keys'   # (dacs.py:850-857)
            names = ['decode.loss_seg', 'decode.acc_seg', 'mix.decode.loss_seg', 'mix.decode.acc_seg'] + (['src.loss_imnet_feat_dist'] if lam else [])
            got = torch.tensor([float(lv[k]) for k in names])
            ref = g[f'{p}.losses'].float()
            tol_l = (1e-4 if exact else 3e-4) * (1 if it == 0 else 10)
            loss_idx = [0, 2] + ([4] if lam else [])
            assert_close(got[loss_idx], ref[loss_idx], tol_l, name=f'{p} losses vs reference')
            check_le(f'{p} accuracies vs reference (points)', (got[[1, 3]] - ref[[1, 3]]).abs().max().item(), 0.1 if it == 0 else 0.5)
            mix = dacs.last_mix
            plab = mix['pseudo_label'].cpu().view(1, 512, 512)[..., ::8, ::8].to(torch.uint8)
            agree = (plab.flatten() == g[f'{p}.pseudo_label_s'].flatten()).float().mean().item()
            check_le(f'{p} pseudo-label disagreement', 1 - agree, 1e-3 if it == 0 else 1e-2)
            check_le(f'{p} confident-pixel count rel', abs(int(mix['pseudo_count'].sum()) - int(g[f'{p}.pseudo_conf'])) /
                     max(1, int(g[f'{p}.pseudo_conf'])), 1e-3 if it == 0 else 1e-2)
            teacher = ops.upsample_logits_nchw(mix['teacher_logits'], 512, 512)   # (the reference's teacher logits are full size)
            assert_close(teacher[..., ::64, ::64], g[f'{p}.teacher_s'], 1e-3 if it == 0 else 1e-2, name=f'{p} teacher logits')
            assert_close(mix['mixed_img'][..., ::16, ::16], g[f'{p}.mixed_img_s'], 1e-3 if gen else 1e-6, name=f'{p} mixed image')
            if gen:
                assert_close(mix['day_image'][..., ::16, ::16], g[f'{p}.src_img_s'], 1e-3, name=f'{p} translated source image')
            mlab = mix['mixed_lbl'].cpu().view(1, 512, 512)[..., ::8, ::8].to(torch.uint8)
            agree = (mlab.flatten() == g[f'{p}.mixed_lbl_s'].flatten()).float().mean().item()
            check_le(f'{p} mixed-label disagreement', 1 - agree, 1e-3 if it == 0 else 1e-2)
            assert_close(mix['pseudo_weight'].view(1, 512, 512)[..., ::8, ::8], g[f'{p}.mixed_weight_s'].view(1, 512 // 8, 512 // 8), 1e-3 if it == 0 else 1e-2, name=f'{p} mixed weight')
            if lam:
                assert int(dacs.debug_fdist_mask.sum()) == int(g[f'{p}.fdist_mask_sum']), f'{p} feature-distance mask size'
            # fingerprints: one row per parameter in the order of g['param_names'] (FP_N samples + sum + abs-sum)
            row = {k: i for i, k in enumerate(g['param_names'])}
            worst_g = max(_fp_rel(sample_grad(q.grad.cpu(), FP_N), g[f'{p}.grad'][row[k]]) for k, q in dacs.model.named_parameters())
            # the bounds of test_fdist.py's step test
            check_le(f'{p} {mode} worst gradient fingerprint error vs reference', worst_g,
                     (1.2e-2 if exact else 3e-2) if it == 0 else (0.3 if exact else 0.4))
            worst_e = max(_fp_rel(sample_grad(q.detach().cpu(), FP_N), g[f'{p}.ema'][row[k]]) for k, q in dacs.ema_model.named_parameters())
            check_le(f'{p} {mode} worst EMA fingerprint error vs reference', worst_e, 1e-3 if it == 0 else 1e-2)
    finally:
        if dacs is not None:
            dacs.inject_draws = None
        rt.set_gemm_x3(False)
        rt.set_compute_dtype(torch.float32)


def _small_batch(tt, B=2, H=64, W=64):
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, 19, (B, 1, H // 32, W // 32), generator=g).repeat_interleave(32, 2).repeat_interleave(32, 3)
    src = dict(image=seeded_randn((B, 3, H, W), 7, 'img'), label=lab)
    tg = {('warp_image' if tt == 'cs2dsec_image' else 'image'): seeded_randn((B, 3, H, W), 7, 'nimg')}
    return src, tg


@pytest.mark.gpu
@pytest.mark.parametrize('tt,lam,gen', [('cs2dsec_image', 0.005, False), ('cs2dz_image', 0.0, True)])
def test_image_graph_replay_matches_eager_gpu(tt, lam, gen):
    """three iterations eager against hipGraph replay (warm-up 1, capture at iteration 1): same losses, same gradients"""
    dev = _gpu().device
    rt.set_compute_dtype(torch.float32)
    src, tg = _small_batch(tt)
    runs = []
    for graph in (False, True):
        dacs = build_train_model(make_cfg(tt, [32, 64, 160, 256], 64, lam=lam, generator=gen))
        seeded_fill(dacs.model, 7)
        seeded_fill(dacs.ema_model, 8)
        if gen:
            seeded_fill(dacs.cyclegan_id2in, 9)
        if lam:
            seeded_fill(dacs.imnet_model, 10)
        dacs.to(dev).train()
        torch.manual_seed(11), random.seed(11), np.random.seed(11)
        if graph:
            dacs.enable_graph(warmup_iters=1)
        batch = dict(source={k: v.to(dev) for k, v in src.items()}, target={k: v.to(dev) for k, v in tg.items()})
        out = []
        for it in range(3):
            for p in dacs.model.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            lv = dacs(**batch)
            torch.cuda.synchronize()
            out.append(({k: float(v) for k, v in lv.items() if 'loss' in k},
                        {n: p.grad.detach().cpu().clone() for n, p in dacs.model.named_parameters()}))
        if graph:
            assert dacs._graph is not None, 'the iteration was not captured'
        runs.append(out)
    for it, ((l_e, g_e), (l_g, g_g)) in enumerate(zip(*runs)):
        assert l_e.keys() == l_g.keys() and all(np.isfinite(v) for v in l_e.values())
        for k in l_e:
            assert_close(torch.tensor([l_g[k]]), torch.tensor([l_e[k]]), 1e-4, name=f'it{it} {k}, graph vs eager')
        worst = max((g_g[n] - q).abs().max().item() / (q.abs().max().item() + 1e-12) for n, q in g_e.items())
        check_le(f'{tt} it{it} worst gradient rel error, graph vs eager', worst, 5e-2, strict=True)


@pytest.mark.gpu
def test_image_grad_ready_hook_gpu():
    """a gradient-ready hook (the data-parallel reducer's entry, runtime.grad_ready_hook) armed around the last backward pass: the
    head and the four encoder stages report once each, what they report is final, and the gradients equal those of a run without it"""
    from cmda_amd import optim
    dev = _gpu().device
    rt.set_compute_dtype(torch.float32)
    src, tg = _small_batch('cs2dsec_image')
    grads = []
    for armed in (False, True):
        dacs = build_train_model(make_cfg('cs2dsec_image', [32, 64, 160, 256], 64, lam=0.005))
        seeded_fill(dacs.model, 7)
        seeded_fill(dacs.ema_model, 8)
        seeded_fill(dacs.imnet_model, 10)
        dacs.to(dev).train()
        opt = optim.FlatAdamW(dacs.model, custom_keys=dict(head=dict(lr_mult=10.0), norm=dict(decay_mult=0.0)))
        dacs.attach_flat_store(opt)
        student = dacs.model
        ranges = {('decode_head', id(student.decode_head)): opt.ranges_of(student, ['decode_head.'], min_elems=0)}
        for s in range(1, 5):
            ranges[(f'backbone.stage{s}', id(student.backbone))] = opt.ranges_of(
                student, [f'backbone.patch_embed{s}.', f'backbone.block{s}.', f'backbone.norm{s}.'], min_elems=0)
        seen, snaps = [], {}

        def hook(tag, module=None):
            seen.append(tag)
            if (tag, id(module)) in ranges:
                snaps[(tag, id(module))] = [opt.flat_g[lo:hi].clone() for lo, hi in ranges[(tag, id(module))]]
        if armed:
            dacs.final_pass_grad_hook = hook
        batch = dict(source={k: v.to(dev) for k, v in src.items()}, target={k: v.to(dev) for k, v in tg.items()})
        torch.manual_seed(11), random.seed(11), np.random.seed(11)
        opt.zero_grad()
        dacs(**batch)
        torch.cuda.synchronize()
        assert rt.grad_ready_hook is None
        if armed:
            assert seen == ['decode_head'] + [f'backbone.stage{s}' for s in (4, 3, 2, 1)] and len(snaps) == 5, seen
            for key, parts in snaps.items():
                for (lo, hi), snap in zip(ranges[key], parts):
                    assert torch.equal(snap, opt.flat_g[lo:hi]), f'{key[0]}: changed after being reported'
        grads.append(opt.flat_g.detach().cpu().clone())
    worst = (grads[1] - grads[0]).abs().max().item() / (grads[0].abs().max().item() + 1e-12)
    check_le('gradients with the hook armed vs without, rel', worst, 1e-5)


@pytest.mark.gpu
def test_image_full_size_bf16_graph_gpu():
    """MiT-B5 at 512 x 512, 2 + 2 samples, bf16, graph replay, FD on: finite losses; the teacher's logits and pseudo-labels of the
    replayed iteration against an f32 eager run of the same weights and inputs (agreement logged and bounded)"""
    dev = _gpu().device
    B, H, W = 2, 512, 512
    g = torch.Generator().manual_seed(21)
    lab = torch.randint(0, 19, (B, 1, H // 32, W // 32), generator=g).repeat_interleave(32, 2).repeat_interleave(32, 3)
    src = dict(image=torch.randn(B, 3, H, W, generator=g), label=lab)
    tg = dict(warp_image=torch.randn(B, 3, H, W, generator=g))
    res = {}
    try:
        for dt in (torch.bfloat16, torch.float32):
            rt.set_compute_dtype(dt)
            dacs = build_train_model(make_cfg('cs2dsec_image', [64, 128, 320, 512], 256, lam=0.005, depths=(3, 6, 40, 3)))
            seeded_fill(dacs.model, 7)
            seeded_fill(dacs.ema_model, 8)
            seeded_fill(dacs.imnet_model, 10)
            with torch.no_grad():
                dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
            dacs.to(dev).train()
            if dt == torch.bfloat16:
                dacs.enable_graph(warmup_iters=1)
            batch = dict(source={k: v.to(dev) for k, v in src.items()}, target={k: v.to(dev) for k, v in tg.items()})
            for it in range(2):
                torch.manual_seed(11 + it), random.seed(11 + it), np.random.seed(11 + it)
                for p in dacs.model.parameters():
                    if p.grad is not None:
                        p.grad.zero_()
                lv = dacs(**batch)
            torch.cuda.synchronize()
            if dt == torch.bfloat16:
                assert dacs._graph is not None
            mix = dacs.last_mix
            res[dt] = ({k: float(v) for k, v in lv.items()}, mix['teacher_logits'].float().cpu(), mix['pseudo_label'].cpu())
            del dacs, mix
            torch.cuda.empty_cache()
    finally:
        rt.set_compute_dtype(torch.float32)
    (lb, tb, pb), (lf, tf, pf) = res[torch.bfloat16], res[torch.float32]
    print('bf16', lb, 'f32', lf)
    assert all(np.isfinite(v) for v in lb.values())
    check_le('full size bf16 vs f32: teacher logits rel', (tb - tf).abs().max().item() / tf.abs().max().item(), 0.1)
    check_le('full size bf16 vs f32: pseudo-label disagreement', (pb != pf).float().mean().item(), 0.05)
    for k in ('decode.loss_seg', 'mix.decode.loss_seg'):
        check_le(f'full size bf16 vs f32: {k} rel', abs(lb[k] - lf[k]) / abs(lf[k]), 0.05)
