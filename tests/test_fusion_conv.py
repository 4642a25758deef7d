"""Module-level tests of the convolutional fusion modules (cmda_amd/fusion.py: ConvertAvgFusion, AverageFusion) against the fixtures
the reference's own modules produced (tests/golden/make_golden_fusion_conv.py: fusion_caf.npz with its _dx / _eval parts,
fusion_af.npz, fusion_conv_keys.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import sample_grad, seeded_fill, seeded_randn  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import fusion as fu  # noqa: E402
from cmda_amd import ops  # noqa: E402
from cmda_amd.registry import build_fusion, build_segmentor  # noqa: E402
from conftest import assert_close, assert_close_fingerprint  # noqa: E402

DIMS, STRIDES = [64, 128, 320, 512], [4, 8, 16, 32]
SEED, B, H, W = 93, 2, 64, 128


def gold(name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', name + '.npz')).items()}


@pytest.fixture
def mode(request, tgt):
    dt = getattr(request, 'param', torch.float32)
    rt.set_compute_dtype(dt)
    yield dt
    rt.set_compute_dtype(torch.float32)


def nlc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def feats(tgt, tag, seed=SEED, b=B, h=H, w=W):
    return [(tgt.to(nlc(seeded_randn((b, c, h // s, w // s), seed, f'{tag}{i}')).to(rt.compute_dtype())), h // s, w // s)
            for i, (c, s) in enumerate(zip(DIMS, STRIDES))]


def dys(tgt):
    return [tgt.to(nlc(seeded_randn((B, c, H // s, W // s), SEED + 1, f'dy{i}')).to(rt.compute_dtype())) for i, (c, s) in enumerate(zip(DIMS, STRIDES))]


# ---------------------------------------------------------------------------------------------- registry
def test_registry_builds_both_modules():
    caf, af = build_fusion(dict(type='ConvertAvgFusion')), build_fusion(dict(type='AverageFusion'))
    assert isinstance(caf, fu.ConvertAvgFusion) and isinstance(af, fu.AverageFusion)
    with open(os.path.join(HERE, 'golden', 'fusion_conv_keys.json')) as f:
        assert sorted(caf.state_dict().keys()) == json.load(f)
    assert not af.state_dict() and not list(af.parameters())
    assert caf.per_pass_statistics and not getattr(af, 'per_pass_statistics', False)
    caf.init_weights(), af.init_weights()


@pytest.mark.parametrize('name', ['cs2dsec_image+events_together_b5', 'cs2dz_image+raw-isr_b5'])
@pytest.mark.parametrize('fusion', ['ConvertAvgFusion', 'AverageFusion'])
def test_golden_configs_build_with_the_fusion_module_replaced(name, fusion):
    with open(os.path.join(HERE, 'golden', 'configs', name + '.json')) as f:
        model = json.load(f)['model']
    model['fusion_module'] = dict(type=fusion)
    for k in ('backbone_image', 'backbone_events'):
        model[k] = dict(model[k], pretrained=None)
    model['pretrained'] = None
    seg = build_segmentor(model)
    assert type(seg.fusion_module).__name__ == fusion


# ---------------------------------------------------------------------------------------------- ConvertAvgFusion against the reference
# bf16 bounds: 2.5x the worst value of the MI355X run (the convention of tests/test_modules.py:59), each relative to its tensor's largest
# element.  A bf16 pre-activation that rounds across zero flips its ReLU mask and moves that element's whole gradient (and, on the 2 x 4
# map of level 4, a visible share of a BatchNorm parameter's), so the gradients are gated like the fp32 ones -- outlier_frac 1e-2 --
# with `dx` / `grad` bounding the other 99 % and `dx_max` / `grad_max` the single worst element.
# Measured: out 5.27e-3, eval 5.27e-3, dx 99th percentile 3.38e-2, dx max 0.632, gradient samples 99th percentile 0.101, max 0.354
# (their sums 1.5e-2 of the abs-sum), running statistics 8.8e-4.
BF16 = dict(out=1.3e-2, eval=1.3e-2, dx=8.5e-2, dx_max=1.6, grad=0.25, grad_max=0.9, running=2.2e-3)


def _figure(worst, key, got, ref, q=None):
    """relative error of got against ref (max, or the q-quantile of the elements) folded into worst[key]; printed by the caller"""
    d = (got.detach().float().cpu() - ref.float()).abs().flatten() / ref.abs().max().item()
    v = d.max().item() if q is None else d.kthvalue(max(1, int(q * d.numel()))).values.item()
    worst[key] = max(worst.get(key, 0.0), v)


@pytest.mark.parametrize('mode', [torch.float32, torch.bfloat16], indirect=True)
def test_convert_avg_fusion_golden(tgt, mode):
    """train-mode forward and backward, then an eval-mode forward, against the reference's module on the same weights and inputs.
    fp32: outputs 1e-4, dx 3e-4 (outlier_frac 1e-2: the allowance test_head_train_golden gives train-mode BN + ReLU), parameter-gradient
    fingerprints 5e-4 (atol 1e-6, same allowance), running statistics 1e-4, eval forward 1e-4.  bf16: see BF16."""
    g, gdx, gev = gold('fusion_caf'), gold('fusion_caf_dx'), gold('fusion_caf_eval')
    m = seeded_fill(fu.ConvertAvgFusion(), SEED).train().to(tgt.device)
    outs, saved = m.fwd(feats(tgt, 'i'), feats(tgt, 'e'), B)
    di, de = m.bwd(saved, dys(tgt), B)
    running = {k: v.clone() for k, v in m.state_dict().items() if 'running' in k}
    m.eval()
    evals, none = m.fwd(feats(tgt, 'i'), feats(tgt, 'e'), B, save=False)
    assert none is None
    f32 = mode == torch.float32
    worst = {}
    for i in range(4):
        _figure(worst, 'out', outs[i][0], nlc(g[f'out{i}']))
        _figure(worst, 'eval', evals[i][0], nlc(gev[f'eval{i}']))
        for tag, d in (('di', di), ('de', de)):
            _figure(worst, 'dx max', d[i], nlc(gdx[f'{tag}{i}']))
            _figure(worst, 'dx 99th percentile', d[i], nlc(gdx[f'{tag}{i}']), 0.99)
    for name, p in m.named_parameters():
        _figure(worst, 'grad sample', sample_grad(p.grad)[:-2], g['grad.' + name][:-2])
        _figure(worst, 'grad sample 99th percentile', sample_grad(p.grad)[:-2], g['grad.' + name][:-2], 0.99)
        _figure(worst, 'grad sums', sample_grad(p.grad)[-2:] / g['grad.' + name][-1], g['grad.' + name][-2:] / g['grad.' + name][-1])
    for k, v in running.items():
        _figure(worst, 'running', v, g['bn.' + k])
    print(f'ConvertAvgFusion {tgt} {mode}: ' + ', '.join(f'{k} {v:.3e}' for k, v in worst.items()))
    for i in range(4):
        assert_close(outs[i][0], nlc(g[f'out{i}']), 1e-4 if f32 else BF16['out'], name=f'out{i}')
        for tag, d in (('di', di), ('de', de)):
            assert_close(d[i], nlc(gdx[f'{tag}{i}']), 3e-4 if f32 else BF16['dx'], name=f'{tag}{i}', outlier_frac=1e-2,
                         outlier_rtol=0.05 if f32 else BF16['dx_max'])
    seen = 0
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        assert_close_fingerprint(sample_grad(p.grad), g['grad.' + name], 5e-4 if f32 else BF16['grad'], atol=1e-6 if f32 else 1e-3,
                                 name='grad.' + name, outlier_frac=1e-2, outlier_rtol=0.05 if f32 else BF16['grad_max'])
        seen += 1
    assert seen == sum(k.startswith('grad.') for k in g) == 48
    for k, v in running.items():
        assert_close(v, g['bn.' + k], 1e-4 if f32 else BF16['running'], name=k)
    for i in range(4):
        assert_close(evals[i][0], nlc(gev[f'eval{i}']), 1e-4 if f32 else BF16['eval'], name=f'eval{i}')


def test_convert_avg_fusion_nchw_forward(tgt):
    """forward(image_features, events_features) on NCHW lists, the reference's interface"""
    g = gold('fusion_caf')
    m = seeded_fill(fu.ConvertAvgFusion(), SEED).train().to(tgt.device)
    fi = [tgt.to(seeded_randn((B, c, H // s, W // s), SEED, f'i{i}')) for i, (c, s) in enumerate(zip(DIMS, STRIDES))]
    fe = [tgt.to(seeded_randn((B, c, H // s, W // s), SEED, f'e{i}')) for i, (c, s) in enumerate(zip(DIMS, STRIDES))]
    for i, o in enumerate(m(fi, fe)):
        assert_close(o, g[f'out{i}'], 1e-4, name=f'out{i}')


# ---------------------------------------------------------------------------------------------- AverageFusion
def test_average_fusion(tgt):
    g = gold('fusion_af')
    m = fu.AverageFusion()
    outs, saved = m.fwd(feats(tgt, 'i'), feats(tgt, 'e'), B)
    for i, (o, _, _) in enumerate(outs):
        assert_close(o, nlc(g[f'out{i}']), 1e-6, name=f'out{i}')
    d = dys(tgt)
    d[2] = None
    di, de = m.bwd(saved, d, B)
    assert di[2] is None and de[2] is None
    for i in (0, 1, 3):
        assert_close(di[i], 0.5 * d[i], 1e-6, name=f'di{i}')
        assert_close(de[i], 0.5 * d[i], 1e-6, name=f'de{i}')
        assert di[i].data_ptr() != de[i].data_ptr() and di[i].data_ptr() != d[i].data_ptr(), 'the halves must be stored separately'
    fi = [tgt.to(seeded_randn((B, c, H // s, W // s), SEED, f'i{i}')) for i, (c, s) in enumerate(zip(DIMS, STRIDES))]
    fe = [tgt.to(seeded_randn((B, c, H // s, W // s), SEED, f'e{i}')) for i, (c, s) in enumerate(zip(DIMS, STRIDES))]
    for i, o in enumerate(m(fi, fe)):
        assert_close(o, g[f'out{i}'], 1e-6, name=f'nchw out{i}')


# ---------------------------------------------------------------------------------------------- per-pass statistics
def _two_pass_feats(tgt, tag):
    """rows laid out pass after pass: pass 0's B samples, then pass 1's (other inputs, shifted so that the passes' statistics differ)"""
    a, b = feats(tgt, tag, SEED), feats(tgt, tag, SEED + 7)
    return a, [(t * 1.5 + 0.5, h, w) for t, h, w in b]


def test_groups_equal_separate_calls(tgt):
    """fwd(..., groups=2) on the rows of two passes equals two separate calls in that order: outputs, saved statistics, the running
    statistics after both, input and parameter gradients"""
    ai, bi = _two_pass_feats(tgt, 'i')
    ae, be = _two_pass_feats(tgt, 'e')
    cat = lambda x, y: [(torch.cat([p[0], q[0]]).contiguous(), p[1], p[2]) for p, q in zip(x, y)]
    d = dys(tgt)
    m1 = seeded_fill(fu.ConvertAvgFusion(), SEED).train().to(tgt.device)
    m2 = seeded_fill(fu.ConvertAvgFusion(), SEED).train().to(tgt.device)
    outs, saved = m1.fwd(cat(ai, bi), cat(ae, be), 2 * B, groups=2)
    di, de = m1.bwd(saved, [torch.cat([x, 2 * x]).contiguous() for x in d], 2 * B)
    o_a, s_a = m2.fwd(ai, ae, B)
    o_b, s_b = m2.fwd(bi, be, B)
    dia, dea = m2.bwd(s_a, d, B)
    dib, deb = m2.bwd(s_b, [2 * x for x in d], B)
    for i in range(4):
        n = outs[i][0].shape[0] // 2
        assert_close(outs[i][0][:n], o_a[i][0], 1e-6, name=f'pass 0 out{i}')
        assert_close(outs[i][0][n:], o_b[i][0], 1e-6, name=f'pass 1 out{i}')
        for br in (0, 2):   # the image-side and the event-side branch: bn2's statistics, then bn1's
            for k in ('mean', 'rstd'):
                assert_close(saved[i][br][k][0], s_a[i][br][k][0], 1e-6, name=f'level {i} bn2 {k}, pass 0')
                assert_close(saved[i][br][k][1], s_b[i][br][k][0], 1e-6, name=f'level {i} bn2 {k}, pass 1')
            for j in (0, 1):
                assert_close(saved[i][br + 1][1][j][0], s_a[i][br + 1][1][j][0], 1e-6, name=f'level {i} bn1 stats {j}, pass 0')
                assert_close(saved[i][br + 1][1][j][1], s_b[i][br + 1][1][j][0], 1e-6, name=f'level {i} bn1 stats {j}, pass 1')
        assert_close(di[i][:n], dia[i], 1e-5, name=f'pass 0 di{i}')
        assert_close(di[i][n:], dib[i], 1e-5, name=f'pass 1 di{i}')
        assert_close(de[i][:n], dea[i], 1e-5, name=f'pass 0 de{i}')
        assert_close(de[i][n:], deb[i], 1e-5, name=f'pass 1 de{i}')
    for (k, v), (_, r) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if 'running' in k:
            assert_close(v, r, 1e-6, name=k)
    for (k, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert_close(p.grad, q.grad, 2e-5, atol=1e-7, name='grad ' + k)


def test_joint_extract_hands_the_pass_count_to_modules_that_ask(tgt, monkeypatch):
    """FusionEncoderDecoder._extract_joint over two passes: a module with `per_pass_statistics` is called with groups=2, any other
    exactly as before"""
    from test_dacs import SMALL, make_cfg
    calls = {}
    for name in ('ConvertAvgFusion', 'AverageFusion', 'AttentionAvgFusion'):
        cfg = make_cfg(SMALL['dims'], SMALL['ch'])['model']
        if name == 'ConvertAvgFusion':
            cfg['fusion_module'] = dict(type=name, in_channels=SMALL['dims'], out_channels=SMALL['dims'])
        elif name == 'AverageFusion':
            cfg['fusion_module'] = dict(type=name)
        seg = build_segmentor(cfg).train().to(tgt.device)
        real = seg.fusion_module.fwd

        def spy(*a, _real=real, _name=name, **kw):
            calls[_name] = dict(kw)
            return _real(*a, **kw)
        monkeypatch.setattr(seg.fusion_module, 'fwd', spy)
        img = [tgt.to(seeded_randn((1, 3, 32, 32), 3, f'img{p}')) for p in range(2)]
        ev = [tgt.to(seeded_randn((1, 3, 32, 32), 3, f'ev{p}')) for p in range(2)]
        with torch.no_grad():
            seg._extract_joint(img, ev, None, False)
    assert calls['ConvertAvgFusion'].get('groups') == 2
    assert 'groups' not in calls['AverageFusion'] and 'groups' not in calls['AttentionAvgFusion']


# ---------------------------------------------------------------------------------------------- into= and the call pattern
@pytest.mark.parametrize('cls', ['ConvertAvgFusion', 'AverageFusion'])
def test_into_slices(tgt, cls):
    m = seeded_fill(getattr(fu, cls)(), SEED).train().to(tgt.device)
    fi, fe = feats(tgt, 'i'), feats(tgt, 'e')
    bufs = [torch.full((3 * t.shape[0], t.shape[1]), float('nan'), dtype=t.dtype, device=tgt.device) for t, _, _ in fi]
    into = [b[t.shape[0]:2 * t.shape[0]] for b, (t, _, _) in zip(bufs, fi)]
    outs, _ = m.fwd(fi, fe, B, into=into)
    ref, _ = seeded_fill(getattr(fu, cls)(), SEED).train().to(tgt.device).fwd(fi, fe, B)
    for i, ((o, _, _), buf) in enumerate(zip(outs, bufs)):
        n = fi[i][0].shape[0]
        assert o.data_ptr() == into[i].data_ptr()
        assert torch.equal(buf[n:2 * n].cpu(), ref[i][0].cpu()), f'level {i}'
        assert torch.isnan(buf[:n]).all().item() and torch.isnan(buf[2 * n:]).all().item()


def test_call_pattern(tgt, monkeypatch):
    """one training forward issues exactly one cmdax8_resavg_fwd, the backward exactly one cmdax8_resavg_bwd; BatchNorm 2 never runs
    an apply pass of its own (eight cmdax8_bn_stats, eight cmda_bn_train_fwd for bn1)"""
    m = seeded_fill(fu.ConvertAvgFusion(), SEED).train().to(tgt.device)
    names = []
    real = ops.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, 'call', spy)
    outs, saved = m.fwd(feats(tgt, 'i'), feats(tgt, 'e'), B)
    fwd_names, names[:] = list(names), []
    m.bwd(saved, dys(tgt), B)
    assert fwd_names.count('cmdax8_resavg_fwd') == 1 and fwd_names.count('cmdax8_bn_stats') == 8
    assert fwd_names.count('cmda_bn_train_fwd') == 8 and fwd_names.count('cmda_axpby') == 0
    assert names.count('cmdax8_resavg_bwd') == 1 and names.count('cmda_bn_train_bwd') == 8 and 'cmdax8_resavg_fwd' not in names
