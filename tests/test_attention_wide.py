"""Fused attention for the fusion modules' wide heads (attention_wide.hip): head dim C / heads in {128, ..., 1024}, walked in 64-wide
chunks by the same scores / softmax / weighted-sum orientation as the head-64 kernels.  The reference builds both fusion modules from the
MiT Block with num_heads = 1 (fusion/attention_avg_fusion.py:27-51: head dims 64 / 128 / 320 / 512; fusion/attention_fusion.py:27-59 on the
concatenated streams: 128 / 256 / 640 / 1024).

The checker is fp32 autograd on the same bf16 inputs.  Bounds: the project's own for this arithmetic (tests/test_kernels.py::
test_fused_attention): 1.6e-2 for o, 2e-2 for dq and dK | dV, max-norm relative.  A torch model of the fused arithmetic (fp32 scores, P and
dS rounded once to bf16, bf16 outputs, fp32 dK | dV) sits at 4.9e-3 / 4.4e-3 / 3.0e-3 or below on exactly these cases.

Which head dims take these kernels BY DEFAULT is a measured table (ops.ATTN_WIDE_TABLE: 128 both ways, 256 forward-only; the wider ones lost
to the GEMM + softmax path on the MI355X at the configs' shapes).  The kernels exist and are held to the bounds for
every head dim, so the tests below select them with CMDA_ATTN_WIDE=2 (every wide head, whatever the table says);
test_wide_default_dispatch_follows_the_table pins what runs without the switch."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import seeded_fill, seeded_randn  # noqa: E402

import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import nn as K  # noqa: E402
from cmda_amd import ops  # noqa: E402
from conftest import Target, assert_close, check_le  # noqa: E402


def _attention_ref(q, kv, B, N, Nk, heads, C, scale):
    hd = C // heads
    qf = q.view(B, N, heads, hd).permute(0, 2, 1, 3)
    k = kv[:, :C].reshape(B, Nk, heads, hd).permute(0, 2, 1, 3)
    v = kv[:, C:].reshape(B, Nk, heads, hd).permute(0, 2, 1, 3)
    a = (qf @ k.transpose(-1, -2) * scale).softmax(-1)  # mix_transformer.py:97-99
    return (a @ v).permute(0, 2, 1, 3).reshape(B * N, C)


def _rel(got, ref):
    return (got.detach().float().cpu() - ref.detach().float()).abs().max().item() / max(ref.detach().abs().max().item(), 1e-30)


def _problem(B, N, Nk, heads, hd, grad=True):
    torch.manual_seed(N + Nk + hd)
    C = heads * hd
    q, kv, do = torch.randn(B * N, C).bfloat16(), torch.randn(B * Nk, 2 * C).bfloat16(), torch.randn(B * N, C).bfloat16()
    qr, kvr = q.float().requires_grad_(grad), kv.float().requires_grad_(grad)
    ref = _attention_ref(qr, kvr, B, N, Nk, heads, C, hd ** -0.5)
    if grad:
        ref.backward(do.float())
    return q, kv, do, ref.detach(), qr.grad, kvr.grad


@pytest.fixture
def all_wide(monkeypatch):
    monkeypatch.setenv('CMDA_ATTN_WIDE', '2')


@pytest.fixture
def bf16_mode():
    rt.set_compute_dtype(torch.bfloat16)
    yield
    rt.set_compute_dtype(torch.float32)


WIDE_CASES = [(1, 64, 256, 1, 128), (2, 200, 256, 2, 128), (1, 70, 37, 1, 320), (1, 300, 130, 1, 512), (2, 1100, 256, 1, 256),
              (1, 70, 4, 1, 128), (1, 130, 256, 1, 640), (1, 96, 256, 1, 1024), (2, 4100, 256, 1, 128)]


@pytest.mark.parametrize('B,N,Nk,heads,hd', WIDE_CASES)
def test_wide_attention(tgt, all_wide, B, N, Nk, heads, hd):
    """o, dq and dK | dV of the chunked kernels against autograd on the same bf16 inputs"""
    if B * N > 8000 and tgt.device.type != 'cuda':
        pytest.skip('the 8200-query case is GPU only (emulator run time), like the largest case of test_fused_attention')
    C, scale = heads * hd, hd ** -0.5
    q, kv, do, ref, dq_ref, dkv_ref = _problem(B, N, Nk, heads, hd)
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    assert ops.attention_fused_ok(qd, Nk, heads, C)
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale)
    assert_close(o, ref, 1.6e-2, name='wide attention o')
    dkv = torch.zeros(B * Nk, 2 * C, device=tgt.device)
    dq = ops.attention_fused_bwd(qd, kvd, dod, dkv, B, N, Nk, heads, C, scale)
    assert_close(dq, dq_ref, 2e-2, name='wide attention dq')
    assert_close(dkv[:, :C], dkv_ref[:, :C], 2e-2, name='wide attention dk')   # (dK and dV each against its own maximum)
    assert_close(dkv[:, C:], dkv_ref[:, C:], 2e-2, name='wide attention dv')


@pytest.mark.parametrize('B,N,Nk,heads,hd', [(1, 100, 280, 1, 320), (1, 90, 260, 1, 128), (1, 280, 280, 1, 512)])
def test_wide_attention_eval_keys(tgt, all_wide, B, N, Nk, heads, hd):
    """the 260 / 280 keys of the 440 x 640 evaluation frames: the forward-only 320-key instance"""
    C, scale = heads * hd, hd ** -0.5
    q, kv, _, ref, _, _ = _problem(B, N, Nk, heads, hd, grad=False)
    qd, kvd = tgt.to(q), tgt.to(kv)
    assert ops.attention_fused_ok(qd, Nk, heads, C, need_grad=False)
    assert not ops.attention_fused_ok(qd, Nk, heads, C, need_grad=True)
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale)
    assert_close(o, ref, 1.6e-2, name='wide attention o (eval keys)')


@pytest.mark.parametrize('B,N,Nk,heads,hd', [(2, 77, 37, 1, 128), (1, 45, 7, 2, 192), (2, 130, 250, 1, 320), (1, 19, 13, 1, 512)])
def test_wide_attention_padding(tgt, all_wide, B, N, Nk, heads, hd):
    """N not a multiple of 16, Nk not a multiple of 16 or 32 (and below 16): nothing outside the valid rows is written (NaN-filled
    outputs keep a canary tail), and no masked key leaks into a valid row"""
    C, scale = heads * hd, hd ** -0.5
    q, kv, do, ref, dq_ref, dkv_ref = _problem(B, N, Nk, heads, hd)
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    tail = 40
    from cmda_amd.ops import call, ptr, c_i32, c_f32, dtype_tag, stream_of
    o = torch.full((B * N + tail, C), float('nan'), dtype=torch.bfloat16, device=tgt.device)
    o[B * N:] = 7.0
    call('cmda_attention_fwd', ptr(qd), ptr(kvd), ptr(o), c_i32(B), c_i32(N), c_i32(Nk), c_i32(heads), c_i32(C), c_f32(scale),
         dtype_tag(qd), stream_of(qd))
    assert torch.isfinite(o[:B * N].float()).all(), 'a valid output row was left unwritten or took a NaN'
    assert (o[B * N:].float() == 7.0).all(), 'the forward wrote past row B * N'
    assert_close(o[:B * N], ref, 1.6e-2, name='wide attention o (ragged)')
    dq = torch.full((B * N + tail, C), float('nan'), dtype=torch.bfloat16, device=tgt.device)
    dq[B * N:] = 7.0
    dkv = torch.zeros(B * Nk + tail, 2 * C, device=tgt.device)
    dkv[B * Nk:] = 7.0
    stats = torch.full((B * N * heads * 2 + tail,), 7.0, device=tgt.device)
    call('cmda_attention_bwd', ptr(qd), ptr(kvd), ptr(dod), ptr(dq), ptr(dkv), ptr(None), ptr(stats), c_i32(B), c_i32(N), c_i32(Nk),
         c_i32(heads), c_i32(C), c_f32(scale), dtype_tag(qd), stream_of(qd))
    assert torch.isfinite(dq[:B * N].float()).all() and (dq[B * N:].float() == 7.0).all(), 'dq rows'
    assert torch.isfinite(dkv).all() and (dkv[B * Nk:] == 7.0).all(), 'dK | dV rows'
    assert torch.isfinite(stats).all() and (stats[B * N * heads * 2:] == 7.0).all(), 'stats'
    assert_close(dq[:B * N], dq_ref, 2e-2, name='wide attention dq (ragged)')
    assert_close(dkv[:B * Nk, :C], dkv_ref[:, :C], 2e-2, name='wide attention dk (ragged)')
    assert_close(dkv[:B * Nk, C:], dkv_ref[:, C:], 2e-2, name='wide attention dv (ragged)')


def test_wide_attention_rejects_direct_only(tgt):
    """there is no direct (bf16-stored) dK | dV mode for wide heads: the entry refuses a call without the fp32 accumulator with
    CMDA_ERR_SHAPE (not CMDA_ERR_UNSUPPORTED: the head dim itself is served) and leaves dkv16 alone; the same call with dkv32 runs"""
    from cmda_amd import _lib
    from cmda_amd.ops import ptr, c_i32, c_f32, dtype_tag, stream_of
    B, N, Nk, C = 1, 64, 64, 128
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=tgt.device)
    q, kv, do, dq, dkv16 = z(B * N, C), z(B * Nk, 2 * C), z(B * N, C), z(B * N, C), z(B * Nk, 2 * C)
    stats = torch.zeros(B * N * 2, device=tgt.device)
    dkv32 = torch.zeros(B * Nk, 2 * C, device=tgt.device)

    def bwd(acc):
        return _lib.lib().cmda_attention_bwd(ptr(q), ptr(kv), ptr(do), ptr(dq), ptr(acc), ptr(dkv16), ptr(stats), c_i32(B), c_i32(N),
                                            c_i32(Nk), c_i32(1), c_i32(C), c_f32(0.1), dtype_tag(q), stream_of(q))

    assert bwd(None) == -1, 'CMDA_ERR_SHAPE expected for a wide head without dkv32'
    assert (dkv16 == 0).all()
    assert bwd(dkv32) == 0
    for hd_bad in (96, 1088):   # not a multiple of 64 / beyond 1024
        assert not ops.attention_fused_ok(q, Nk, 1, hd_bad)


def test_wide_default_dispatch_follows_the_table(tgt, bf16_mode, monkeypatch):
    """without CMDA_ATTN_WIDE the measured table decides: head dim 128 runs fused both ways (no probabilities saved), 256 forward-only,
    512 stays on GEMM + softmax; 2 selects the wide kernels for all of them, 0 for none"""
    monkeypatch.delenv('CMDA_ATTN_WIDE', raising=False)
    q = torch.zeros(1, 1, dtype=torch.bfloat16)
    want = ops.ATTN_WIDE_TABLE
    assert want[128] == (True, True) and want[512] == (False, False)   # what the behavioural half below relies on
    for hd, (f, fb) in want.items():
        assert ops.attention_fused_ok(q, 256, 1, hd, need_grad=False) == f and ops.attention_fused_ok(q, 256, 1, hd) == fb, hd
    B, N, Nk = 1, 70, 37
    for hd, fused in ((128, True), (512, False)):
        qd, kvd = tgt.to(torch.randn(B * N, hd).bfloat16()), tgt.to(torch.randn(B * Nk, 2 * hd).bfloat16())
        assert (K.attention_fwd(qd, kvd, B, N, Nk, 1, hd, hd ** -0.5)[1] is None) == fused, hd
    monkeypatch.setenv('CMDA_ATTN_WIDE', '2')
    assert all(ops.attention_fused_ok(q, 256, 1, hd) for hd in want)
    monkeypatch.setenv('CMDA_ATTN_WIDE', '0')
    assert not any(ops.attention_fused_ok(q, 256, 1, hd, need_grad=False) for hd in want)
    assert ops.attention_fused_ok(q, 256, 1, 64)


@pytest.mark.parametrize('B,N,Nk,heads,hd', [(2, 200, 256, 2, 128), (1, 300, 130, 1, 512), (1, 130, 256, 1, 640)])
def test_wide_fused_vs_unfused(tgt, bf16_mode, monkeypatch, B, N, Nk, heads, hd):
    """nn.attention_fwd / attention_bwd with the chunked kernels and with CMDA_ATTN_WIDE=0 (GEMM + softmax, scores rounded to bf16), both
    against fp32 autograd: the fused path has strictly fewer roundings, so its error may exceed the unfused one's by the summation-order
    margin only (factor 1.5)"""
    C, scale = heads * hd, hd ** -0.5
    q, kv, do, ref, dq_ref, dkv_ref = _problem(B, N, Nk, heads, hd)
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)

    def run():
        o, P = K.attention_fwd(qd, kvd, B, N, Nk, heads, C, scale)
        dq, dkv = K.attention_bwd(dod, qd, kvd, P, B, N, Nk, heads, C, scale)
        return P, (_rel(o, ref), _rel(dq, dq_ref), _rel(dkv, dkv_ref))

    monkeypatch.setenv('CMDA_ATTN_WIDE', '2')
    P, fused = run()
    assert P is None, 'the wide head did not take the fused kernels'
    monkeypatch.setenv('CMDA_ATTN_WIDE', '0')
    P, unfused = run()
    assert P is not None and tuple(P.shape) == (B, heads, N, Nk)
    monkeypatch.setenv('CMDA_ATTN_WIDE', '2')
    monkeypatch.setenv('CMDA_NO_FUSED_ATTENTION', '1')
    assert K.attention_fwd(qd, kvd, B, N, Nk, heads, C, scale)[1] is not None, 'CMDA_NO_FUSED_ATTENTION covers every head dim'
    for name, f, u in zip(('o', 'dq', 'dkv'), fused, unfused):
        print(f'{name}: fused {f:.3e} unfused {u:.3e}')
        check_le(f'fused {name} error against 1.5 x unfused', f, 1.5 * u)


def _no_probability_tensor(obj, where='saved'):
    if torch.is_tensor(obj):
        assert obj.dim() != 4, f'{where}: a {tuple(obj.shape)} tensor is kept for the backward'
    elif isinstance(obj, (tuple, list)):
        for i, x in enumerate(obj):
            _no_probability_tensor(x, f'{where}[{i}]')
    elif isinstance(obj, dict):
        for k, x in obj.items():
            _no_probability_tensor(x, f'{where}[{k}]')
    elif hasattr(obj, '__dict__') and not isinstance(obj, (torch.nn.Module, type)):   # an object carrying tensors as attributes
        _no_probability_tensor(vars(obj), where)


def _fusion_errors(tgt, name):
    """forward + backward of one fusion module in bf16 mode at the sizes of test_modules.py::test_fusion_modules_golden -> (worst output
    error against the golden file, worst input-gradient error against the oracle, saved state)"""
    from cmda_amd import fusion as fu
    from oracle import fusion as ofu
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', f'fusion_{name}.npz')).items()}
    dims, strides = [64, 128, 320, 512], [4, 8, 16, 32]
    m = seeded_fill((fu.AttentionAvgFusion if name == 'avg' else fu.AttentionFusion)(drop_path_rate=0.0), 91).train().to(tgt.device)

    def feats(tag):
        out = []
        for i, (c, s) in enumerate(zip(dims, strides)):
            f = seeded_randn((1, c, 64 // s, 64 // s), 91, f'{tag}{i}')
            out.append((tgt.to(f.permute(0, 2, 3, 1).reshape(-1, c).contiguous().to(rt.compute_dtype())), 64 // s, 64 // s))
        return out

    outs, saved = m.fwd(feats('i'), feats('e'), 1)
    e_out = max(_rel(o, g[f'out{i}'].permute(0, 2, 3, 1).reshape(H * W, -1)) for i, (o, H, W) in enumerate(outs))
    ref = seeded_fill((ofu.AttentionAvgFusion if name == 'avg' else ofu.AttentionFusion)(drop_path_rate=0.0), 91).train()
    ri = [seeded_randn((1, c, 64 // s, 64 // s), 91, f'i{k}').requires_grad_(True) for k, (c, s) in enumerate(zip(dims, strides))]
    re = [seeded_randn((1, c, 64 // s, 64 // s), 91, f'e{k}').requires_grad_(True) for k, (c, s) in enumerate(zip(dims, strides))]
    routs = ref(ri, re)
    dys = [seeded_randn(o.shape, 92, f'dy{k}') for k, o in enumerate(routs)]
    sum((o * d).sum() for o, d in zip(routs, dys)).backward()
    dfused = [tgt.to(d.permute(0, 2, 3, 1).reshape(-1, d.shape[1]).contiguous().to(rt.compute_dtype())) for d in dys]
    di, de = m.bwd(saved, dfused, 1)
    ops.gemm_flush_deferred()
    e_grad = max(max(_rel(di[k], ri[k].grad.permute(0, 2, 3, 1).reshape(-1, dims[k])),
                     _rel(de[k], re[k].grad.permute(0, 2, 3, 1).reshape(-1, dims[k]))) for k in range(4))
    return e_out, e_grad, saved


@pytest.mark.parametrize('name', ['avg', 'cat'])
def test_fusion_modules_bf16_fused(tgt, bf16_mode, monkeypatch, name):
    """AttentionAvgFusion / AttentionFusion in bf16 mode with CMDA_ATTN_WIDE=2: every block's attention runs fused (the softmax kernels are never launched, no
    [B, heads, N, Nk] tensor is saved), and outputs / input gradients are no further from the golden file / the oracle than 1.5 x the
    GEMM + softmax path's (CMDA_ATTN_WIDE=0) in the same test.  Measured pairs (fused | unfused): DESIGN.md, wide-head attention."""
    monkeypatch.setenv('CMDA_ATTN_WIDE', '0')
    u_out, u_grad, _ = _fusion_errors(tgt, name)
    monkeypatch.setenv('CMDA_ATTN_WIDE', '2')

    def boom(*a, **k):
        raise AssertionError('a softmax kernel was launched: an attention call left the fused path')

    monkeypatch.setattr(ops, 'softmax_fwd_', boom)
    monkeypatch.setattr(ops, 'softmax_bwd_', boom)
    f_out, f_grad, saved = _fusion_errors(tgt, name)
    _no_probability_tensor(saved)
    print(f'fusion_{name} bf16: outputs fused {f_out:.3e} unfused {u_out:.3e}; input gradients fused {f_grad:.3e} unfused {u_grad:.3e}')
    check_le(f'fusion_{name} outputs: fused against 1.5 x unfused', f_out, 1.5 * u_out)
    check_le(f'fusion_{name} input gradients: fused against 1.5 x unfused', f_grad, 1.5 * u_grad)


@pytest.mark.gpu
def test_fusion_simple_test_440x640_wide_fused(monkeypatch):
    """FusionEncoderDecoder at the 440 x 640 evaluation size in bf16 (depth 1 per stage): the fusion blocks' attention (260 keys at head
    dim 128, 280 at 320 / 512) runs the forward-only 320-key wide instances under CMDA_ATTN_WIDE=2 -- no softmax launch anywhere --, and the logits are no
    further from the fp32 oracle than 1.5 x those of the GEMM + softmax path"""
    from cmda_amd import _lib
    from cmda_amd.registry import build_segmentor
    from oracle import fusion as ofu, head as ohd, mit as omit, segmentor as oseg
    from test_fullsize import DECODER, DIMS, HEAD
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    tgt = Target('gpu')
    bbc = dict(type='MixVisionTransformer', patch_size=4, embed_dims=DIMS, num_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4], qkv_bias=True,
               norm_layer=__import__('functools').partial(torch.nn.LayerNorm, eps=1e-6), depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
               drop_path_rate=0.1)
    head = dict(type='DAFormerHeadFusion', dropout_ratio=0.1,
                decoder_params=dict(DECODER, train_type='cs2dsec_image+events_together', share_decoder=True), **HEAD)
    model = build_segmentor(dict(type='FusionEncoderDecoder', backbone_image=dict(bbc), backbone_events=dict(bbc),
                                 fusion_module=dict(type='AttentionAvgFusion', in_channels=DIMS, drop_path_rate=0.1),
                                 decode_head=head, train_type='cs2dsec_image+events_together', test_cfg=dict(mode='whole')))
    torch.manual_seed(7)
    model.init_weights()
    okw = dict(embed_dims=(64, 128, 320, 512), num_heads=(1, 2, 5, 8), depths=(1, 1, 1, 1), sr_ratios=(8, 4, 2, 1), qkv_bias=True,
               drop_path_rate=0.1)
    ref = oseg.FusionEncoderDecoder(backbone_image=omit.MixVisionTransformer(**okw), backbone_events=omit.MixVisionTransformer(**okw),
                                    fusion_module=ofu.AttentionAvgFusion(drop_path_rate=0.1),
                                    decode_head=ohd.DAFormerHeadFusion(dropout_ratio=0.1, share_decoder=True))
    ref.load_state_dict(model.state_dict())
    model.to(tgt.device).eval()
    ref.eval()
    img = seeded_randn((1, 3, 440, 640), 7, 'img')
    ev = seeded_randn((1, 3, 440, 640), 7, 'ev').clamp(-1, 1)
    meta = dict(ori_shape=(440, 640, 3), img_shape=(440, 640, 3), flip=False)
    with torch.no_grad():
        want = ref.encode_decode(img, ev, test_cfg={'output_type': 'fusion'})
    seen = []
    fused_fwd = ops.attention_fused_fwd

    def spy(q, kv, B, N, Nk, heads, C, scale):
        seen.append((Nk, C // heads))
        return fused_fwd(q, kv, B, N, Nk, heads, C, scale)

    rt.set_compute_dtype(torch.bfloat16)
    try:
        monkeypatch.setenv('CMDA_ATTN_WIDE', '0')
        unfused = model.encode_decode(tgt.to(img), tgt.to(ev), test_cfg={'output_type': 'fusion'}).float().cpu()
        monkeypatch.setenv('CMDA_ATTN_WIDE', '2')
        monkeypatch.setattr(ops, 'attention_fused_fwd', spy)
        monkeypatch.setattr(ops, 'softmax_fwd_', lambda *a, **k: (_ for _ in ()).throw(AssertionError('softmax launched')))
        fused = model.encode_decode(tgt.to(img), tgt.to(ev), test_cfg={'output_type': 'fusion'}).float().cpu()
        pred = model.simple_test(True, warp_image=tgt.to(img), events_vg=tgt.to(ev), img_metas=meta)[0]
    finally:
        rt.set_compute_dtype(torch.float32)
    assert pred.shape == (440, 640)
    for want_inst in ((260, 128), (280, 320), (280, 512)):
        assert want_inst in seen, f'the wide instance (keys, head dim) = {want_inst} was not reached: {sorted(set(seen))}'
    ef, eu = _rel(fused, want), _rel(unfused, want)
    print(f'440x640 fusion logits (bf16, depth 1): fused {ef:.3e} unfused {eu:.3e}')
    check_le('440x640 logits: fused against 1.5 x unfused', ef, 1.5 * eu)
