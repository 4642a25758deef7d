"""Range and launch-regime tests of the kernels that exponentiate or normalise a row: fused attention (bf16, split-bf16, wide heads,
the GEMM + softmax path), softmax.hip, LayerNorm, cross-entropy / pseudo-labels with up-sampling, and GELU over its whole range.

Every reference is float64 and written out here.  The inputs are the families the rest of the suite never feeds: logits far outside
ln(FLT_MAX) = 88.7 in both directions, one-hot probabilities, rows whose mean dwarfs their spread; and the launch regimes production
takes but no other kernel-level test reaches (two-pass forward blocks, the softmax grid-stride loop, the unstaged cross-entropy tile).
A kernel that drops its row maximum, centres after squaring, or mis-addresses one key row fails here and nowhere else in the suite.

Constants named *_K follow the rule of test_kernels.py::_BN_COND_K: 4 x the larger of the emulator and the MI355X measurement, both
quoted where the constant is defined (and in DESIGN.md section 3)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import cmda_amd.runtime as rt
from cmda_amd import _lib as L
from cmda_amd import nn as K
from cmda_amd import ops
from conftest import assert_close, check_le

_F32, _BF16 = torch.float32, torch.bfloat16
_EPS24 = 2.0 ** -24


def _rel_le(name, got, ref, tol, scale=None):
    """max |got - ref| relative to `scale` (default: max |ref|) under tol, through the margin log"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    scale = max(ref.abs().max().item() if scale is None else scale, 1e-30)
    err = (got - ref).abs().max().item() / scale
    check_le(name, err, tol)
    return err


# ====================================================================================================================== attention
# Input families (bf16-exact where the kernel is bf16):
#   randn    today's input, the baseline.
#   shifted  randn, then in the first column of every head q = c_i in {-cq, 0, cq} per query and k = 2: every logit of query i moves
#            by scale * 2 * c_i = +-128 (head dim 64: cq = 512; 256: cq = 1024; 128: cq = 768 -> +-135.8).  exp overflows without the
#            row maximum and the normalisation is 0 / 0 with it dropped; softmax is shift-invariant, so P and all four outputs stay
#            those of a generic case.  dK's shift column (sum_i dS_ij c_i) is far larger than the other 63 and dq's (2 scale sum_j
#            dS_ij) cancels to 0, so each is judged on its own scale: dK's against its own maximum, dq's against the size of the
#            terms that cancel, 2 scale sum_j |dS_ij|.
#   onehot   keys are random +-3 sign vectors, q_i = (4 / 3) k_pi(i) with pi onto every key index: the matching logit is
#            0.125 * 12 * 64 = 96, the others N(0, 12^2), P one-hot to ~e^-50.  o = v[pi] addresses every key row, head offset and
#            batch offset exactly; dq and dK are ~0 in the reference (so: finite and below the absolute tolerance of the randn case
#            of the same shape), dV = scatter of dO.
_SHIFT_Q = {64: 512.0, 128: 768.0, 256: 1024.0}

# Bounds: the suite's own (test_fused_attention*, test_wide_attention) -- bf16 1.6e-2 for o and 2e-2 for gradients, split-bf16 1e-4 and
# 2e-4, each relative to max |ref| of that output.  The split-bf16 kernels under the shifted family add the fp32 spacing of
# scale * s - lse at |shift| = 128 to every probability, so that family's bound is existing + _X3_SHIFT_K * 2^-24 * |shift|.
# Worst err / (2^-24 |shift|) over o, dq, dK, dV and the shifted cases below against float64: 7.97 on the emulator ((1, 1025, 70, 1)),
# 5.06 on an MI355X; _X3_SHIFT_K = 4 x the larger.
_X3_SHIFT_K = 32.0
_ATTN_TOL = {_BF16: (1.6e-2, 2e-2), _F32: (1e-4, 2e-4)}


@functools.lru_cache(maxsize=None)
def _attn_problem(family, B, N, Nk, heads, hd, bf16, grad=True):
    """inputs (q, kv, do, pi) and the float64 reference of one case; computed once, shared by the emulator and the GPU run"""
    gen = torch.Generator().manual_seed(1000 * N + 10 * Nk + heads + hd + len(family))
    C, scale = heads * hd, hd ** -0.5
    q, kv, do = (torch.randn(r, c, generator=gen) for r, c in ((B * N, C), (B * Nk, 2 * C), (B * N, C)))
    pi = None
    if family == 'shifted':
        sign = torch.randint(0, 3, (B * N, 1), generator=gen).float() - 1.0
        q[:, 0::hd] = sign * _SHIFT_Q[hd]
        kv[:, 0:C:hd] = 2.0
    elif family == 'onehot':
        assert N >= Nk and hd == 64
        keys = (torch.randint(0, 2, (B, Nk, heads, hd), generator=gen).float() * 2 - 1) * 3
        pi = torch.stack([torch.cat([torch.randperm(Nk, generator=gen), torch.randint(0, Nk, (N - Nk,), generator=gen)])
                          [torch.randperm(N, generator=gen)] for _ in range(B * heads)]).view(B, heads, N)
        kv[:, :C] = keys.reshape(B * Nk, C)
        q = (keys.permute(0, 2, 1, 3).gather(2, pi[..., None].expand(B, heads, N, hd)) * (4.0 / 3.0)).permute(0, 2, 1, 3).reshape(B * N, C)
    else:
        assert family == 'randn'
    if bf16:
        q, kv, do = q.bfloat16(), kv.bfloat16(), do.bfloat16()
    q4, do4 = q.double().view(B, N, heads, hd), do.double().view(B, N, heads, hd)
    k4, v4 = kv[:, :C].double().view(B, Nk, heads, hd), kv[:, C:].double().view(B, Nk, heads, hd)
    P = (torch.einsum('bnhd,bmhd->bhnm', q4, k4) * scale).softmax(-1)      # mix_transformer.py:97-99
    ref = dict(o=torch.einsum('bhnm,bmhd->bnhd', P, v4).reshape(B * N, C))
    if grad:
        dP = torch.einsum('bnhd,bmhd->bhnm', do4, v4)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        ref['dv'] = torch.einsum('bhnm,bnhd->bmhd', P, do4).reshape(B * Nk, C)
        ref['dq'] = (torch.einsum('bhnm,bmhd->bnhd', dS, k4) * scale).reshape(B * N, C)
        ref['dk'] = (torch.einsum('bhnm,bnhd->bmhd', dS, q4) * scale).reshape(B * Nk, C)
        ref['dq_cancel'] = (torch.einsum('bhnm,bmh->bnh', dS.abs(), k4[..., 0].abs()) * scale).max().item()
        # the size of the terms dS is the difference of, carried through to dq and dK: the scale of a reference that cancels to 0
        T = P * (dP.abs() + (P * dP).sum(-1, keepdim=True).abs())
        ref['dq_terms'] = (torch.einsum('bhnm,bmhd->bnhd', T, k4.abs()) * scale).max().item()
        ref['dk_terms'] = (torch.einsum('bhnm,bnhd->bmhd', T, q4.abs()) * scale).max().item()
    if pi is not None:
        ref['v_pi'] = v4.permute(0, 2, 1, 3).gather(2, pi[..., None].expand(B, heads, N, hd)).permute(0, 2, 1, 3).reshape(B * N, C)
    return q, kv, do, ref


def _grad_scale(ref, name, cols):
    """max |ref| of a gradient -- unless the reference cancels to (near) 0 against its own terms, as dq and dK do with ONE key (P = 1,
    dS = 0 exactly): then the size of those terms, the only scale an absolute error can be held against"""
    m = ref[name][:, cols].abs().max().item()
    return m if m >= 1e-3 * ref[name + '_terms'] else ref[name + '_terms']


def _check_attn_outputs(tag, family, dt, B, N, Nk, heads, hd, ref, o=None, dq=None, dk=None, dv=None):
    """o / dq / dK / dV of one launch against the float64 reference, per family (dK and dV always judged separately)"""
    C = heads * hd
    tol_o, tol_g = _ATTN_TOL[dt]
    shift = 2.0 * _SHIFT_Q[hd] * hd ** -0.5 if family == 'shifted' else 0.0
    extra = _X3_SHIFT_K * _EPS24 * shift if dt == _F32 else 0.0
    col = torch.zeros(C, dtype=torch.bool)
    col[0::hd] = family == 'shifted'
    errs = []
    if family == 'onehot':
        randn_ref = _attn_problem('randn', B, N, Nk, heads, hd, dt == _BF16)[3]
        if o is not None:
            if dt == _BF16:
                assert torch.equal(o.float().cpu(), ref['v_pi'].float()), f'{tag}: o is not bit for bit v[pi]'
            # split-bf16: v = hi + lo carries 16 mantissa bits, so o - v[pi] is at most 2^-17 |v| = 7.6e-6 |v| per element (1.5e-5
            # measured on the emulator at |v| max 4.5); 2^-15 of max |v| is 4 x that rounding
            _rel_le(f'{tag} o (one-hot, vs v[pi])', o, ref['v_pi'], 2.0 ** -15 if dt == _F32 else 0.0)
        for name, got in (('dq', dq), ('dk', dk)):
            if got is not None:
                _rel_le(f'{tag} {name} (one-hot: ~0, absolute)', got, ref[name], tol_g, scale=randn_ref[name].abs().max().item())
        if dv is not None:
            _rel_le(f'{tag} dv (one-hot)', dv, ref['dv'], tol_g)
        return
    if o is not None:
        errs.append(_rel_le(f'{tag} o', o, ref['o'], tol_o + extra))
    if dq is not None:
        errs.append(_rel_le(f'{tag} dq', dq[:, ~col], ref['dq'][:, ~col], tol_g + extra, scale=_grad_scale(ref, 'dq', ~col)))
        if family == 'shifted':
            errs.append(_rel_le(f'{tag} dq (shift column, vs the cancelling terms)', dq[:, col], ref['dq'][:, col], tol_g + extra,
                                scale=ref['dq_cancel']))
    if dk is not None:
        errs.append(_rel_le(f'{tag} dk', dk[:, ~col], ref['dk'][:, ~col], tol_g + extra, scale=_grad_scale(ref, 'dk', ~col)))
        if family == 'shifted':
            errs.append(_rel_le(f'{tag} dk (shift column)', dk[:, col], ref['dk'][:, col], tol_g + extra, scale=_grad_scale(ref, 'dk', col)))
    if dv is not None:
        errs.append(_rel_le(f'{tag} dv', dv, ref['dv'], tol_g + extra))
    if family == 'shifted' and dt == _F32 and errs:
        print(f'{tag} {(B, N, Nk, heads)}: worst err / (2^-24 |shift|) = {max(errs) / (_EPS24 * shift):.3f}')


def _run_fused(tgt, family, dt, B, N, Nk, heads, hd=64, direct_expected=None):
    """forward, dq, dK | dV accumulating and -- where the library takes it -- direct, all against float64"""
    C, scale = heads * hd, hd ** -0.5
    q, kv, do, ref = _attn_problem(family, B, N, Nk, heads, hd, dt == _BF16)
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    assert ops.attention_fused_ok(qd, Nk, heads, C, x3=dt == _F32)
    tag = f'{"bf16" if dt == _BF16 else "split-bf16"} attention [{family}]'
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale)
    assert o.dtype == dt
    dkv = torch.zeros(B * Nk, 2 * C, device=tgt.device)
    dq = ops.attention_fused_bwd(qd, kvd, dod, dkv, B, N, Nk, heads, C, scale)   # accumulating form: fp32 atomics
    _check_attn_outputs(tag, family, dt, B, N, Nk, heads, hd, ref, o, dq, dkv[:, :C], dkv[:, C:])
    direct = hd == 64 and ops.attention_bwd_direct(B, N, Nk, heads)
    if direct_expected is not None:
        assert direct == direct_expected, 'attention_bwd_direct flips between 1024 and 1025 queries'
    if direct:   # one block per key slice stores dK | dV (bf16, or fp32 for split-bf16); NaN on entry: every element must be written
        dkv2 = torch.full((B * Nk, 2 * C), float('nan'), dtype=dt, device=tgt.device)
        dq2 = ops.attention_fused_bwd(qd, kvd, dod, None, B, N, Nk, heads, C, scale, dkv16=dkv2)
        _check_attn_outputs(tag + ' (direct)', family, dt, B, N, Nk, heads, hd, ref, None, dq2, dkv2[:, :C], dkv2[:, C:])


_FAMILIES2 = ['randn', 'shifted']
_DTYPES = [pytest.param(_BF16, id='bf16'), pytest.param(_F32, id='split_bf16')]

# forward / dq blocks of 128 queries (two passes over 64, K / V loaded once) and the shape just below the switch.
#   bf16: 128 per block from 1024 blocks of 128 up.  (64, 130, 20, 8): 2 * 8 * 64 = 1024 blocks, the second of each pair holds 2
#         queries (its second pass is empty); (63, 130, 20, 8): 3 * 8 * 63 = 1512 blocks of 64.
#   split-bf16: from 256 blocks up.  (16, 130, 20, 8): 256 blocks of 128; (15, 130, 20, 8): 3 * 8 * 15 = 360 blocks of 64.
# dK | dV: 4 key-slice blocks per (batch, head) whatever Nk -- 20 keys leave three of them empty.
_QPB = [pytest.param(_BF16, 64, 130, 20, 8, id='bf16-128'), pytest.param(_BF16, 63, 130, 20, 8, id='bf16-64'),
        pytest.param(_F32, 16, 130, 20, 8, id='split_bf16-128'), pytest.param(_F32, 15, 130, 20, 8, id='split_bf16-64')]


@pytest.mark.parametrize('family', _FAMILIES2)
@pytest.mark.parametrize('dt,B,N,Nk,heads', _QPB)
def test_attention_two_pass_blocks(tgt, dt, B, N, Nk, heads, family):
    """the 128-queries-per-block launch of the forward and dq kernels and the 64-per-block launch next to it, at 20 keys"""
    _run_fused(tgt, family, dt, B, N, Nk, heads)


# dK | dV launch regimes (one batch, one head: 2 key slices with 70 keys -- 4 blocks, never a multiple of 8):
#   N = 512 / 513    direct, 4 waves / 8 waves (bf16; split-bf16 has the 4-wave kernel only)
#   N = 1024 / 1025  direct -> accumulating: attention_bwd_direct flips, pinned below.  1025 queries, 70 keys: slices = 2, so
#                    spans = 256 -> 128 queries each -> 9 spans, the last holding 1 query (36 blocks)
# forward / dq: 8, 9, 16, 17 blocks of 64.
@pytest.mark.parametrize('family', _FAMILIES2)
@pytest.mark.parametrize('dt', _DTYPES)
@pytest.mark.parametrize('N', [512, 513, 1024, 1025])
def test_attention_dkv_regimes(tgt, N, dt, family):
    _run_fused(tgt, family, dt, 1, N, 70, 1, direct_expected=N <= 1024)


# key slices of 64: one key, a ragged first slice, exactly one, one over, a ragged third, a ragged fourth, all full.  (1, 70, Nk, 3):
# forward / dq 2 * 3 = 6 blocks, dK | dV 3 * 4 = 12 blocks -- neither a multiple of 8 (xcd_logical_block's remainder path).
@pytest.mark.parametrize('family', _FAMILIES2)
@pytest.mark.parametrize('dt', _DTYPES)
@pytest.mark.parametrize('Nk', [1, 63, 64, 65, 130, 255, 256])
def test_attention_key_slices(tgt, Nk, dt, family):
    _run_fused(tgt, family, dt, 1, 70, Nk, 3)


@pytest.mark.parametrize('family', _FAMILIES2)
@pytest.mark.parametrize('Nk', [257, 320])
def test_attention_eval_keys_forward(tgt, Nk, family):
    """attn_fwd_kernel<320>, forward only: the first key count that takes it and the last it holds (6 blocks)"""
    B, N, heads, C = 1, 70, 3, 192
    q, kv, _, ref = _attn_problem(family, B, N, Nk, heads, 64, True, False)
    qd, kvd = tgt.to(q), tgt.to(kv)
    assert ops.attention_fused_ok(qd, Nk, heads, C, need_grad=False) and not ops.attention_fused_ok(qd, Nk, heads, C)
    o = ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, 0.125)
    _check_attn_outputs(f'bf16 attention, eval keys [{family}]', family, _BF16, B, N, Nk, heads, 64, ref, o)


@pytest.mark.parametrize('dt', _DTYPES)
def test_attention_one_hot_addressing(tgt, dt):
    """P one-hot: o = v[pi] (bit for bit in bf16) over every key row, head and batch; dV = scatter of dO; dq, dK ~ 0 and finite"""
    _run_fused(tgt, 'onehot', dt, 2, 300, 256, 2)


@pytest.mark.parametrize('dt', _DTYPES)
def test_attention_dkv32_accumulates(tgt, dt):
    """dkv32 is documented as accumulated: entering with non-zero contents it leaves as initial + gradient.  (1, 130, 65, 3) takes the
    accumulating form because no direct buffer is passed: 6 key slices -> 128 queries per span -> 2 spans, 24 blocks"""
    B, N, Nk, heads, C = 1, 130, 65, 3, 192
    q, kv, do, ref = _attn_problem('randn', B, N, Nk, heads, 64, dt == _BF16)
    init = torch.randn(B * Nk, 2 * C, generator=torch.Generator().manual_seed(3))
    dkv = tgt.to(init.clone())
    ops.attention_fused_bwd(tgt.to(q), tgt.to(kv), tgt.to(do), dkv, B, N, Nk, heads, C, 0.125)
    tol = _ATTN_TOL[dt][1]
    # (the bound stays relative to the gradient alone: the initial contents add one fp32 rounding of the sum, 6e-8 of it)
    _rel_le('attention dk into non-zero dkv32', dkv[:, :C], init[:, :C].double() + ref['dk'], tol, scale=ref['dk'].abs().max().item())
    _rel_le('attention dv into non-zero dkv32', dkv[:, C:], init[:, C:].double() + ref['dv'], tol, scale=ref['dv'].abs().max().item())


@pytest.mark.parametrize('family', _FAMILIES2)
@pytest.mark.parametrize('B,N,Nk,heads,hd', [(1, 70, 37, 1, 128), (2, 130, 70, 1, 128), (1, 70, 37, 1, 256), (1, 130, 256, 3, 128)])
def test_attention_wide_heads(tgt, monkeypatch, B, N, Nk, heads, hd, family):
    """the chunked kernels of attention_wide.hip at head dims 128 and 256 (CMDA_ATTN_WIDE=2: whatever the dispatch table says);
    accumulating dK | dV only.  Blocks: 2, 6, 2, 9."""
    monkeypatch.setenv('CMDA_ATTN_WIDE', '2')
    _run_fused(tgt, family, _BF16, B, N, Nk, heads, hd)


@pytest.mark.parametrize('dt,family', [pytest.param(_BF16, 'randn', id='bf16-randn'), pytest.param(_F32, 'randn', id='split_bf16-randn'),
                                       pytest.param(_F32, 'shifted', id='split_bf16-shifted')])
def test_attention_unfused_path(tgt, monkeypatch, dt, family):
    """the GEMM + softmax path through nn.attention_fwd / attention_bwd against the same float64 reference.  In bf16 that path STORES
    the scores q k^T as bf16 before the softmax: at |logit| = 128 their spacing is 1, an O(1) error in every logit, so the shifted
    family is outside what its storage format represents (the fused kernels keep the scores in fp32 registers) and only the fp32
    storage of the split-bf16 mode runs it."""
    B, N, Nk, heads, C = 2, 70, 37, 3, 192
    q, kv, do, ref = _attn_problem(family, B, N, Nk, heads, 64, dt == _BF16)
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    rt.set_compute_dtype(dt)
    try:
        if dt == _F32:
            rt.set_gemm_x3(True)
            ops.ATTN_X3_OFF = True
        else:
            monkeypatch.setenv('CMDA_NO_FUSED_ATTENTION', '1')
        o, P = K.attention_fwd(qd, kvd, B, N, Nk, heads, C, 0.125)
        assert P is not None, 'the fused kernel ran'
        dq, dkv = K.attention_bwd(dod, qd, kvd, P, B, N, Nk, heads, C, 0.125)
    finally:
        ops.ATTN_X3_OFF = False
        rt.set_gemm_x3(False)
        rt.set_compute_dtype(_F32)
    _check_attn_outputs(f'unfused {"bf16" if dt == _BF16 else "split-bf16"} attention [{family}]', family, dt, B, N, Nk, heads, 64, ref,
                        o, dq, dkv[:, :C], dkv[:, C:])


# ====================================================================================================================== softmax.hip
# fp32: the worst |p - ref| / max |ref| and |ds - ref| / max |ref| over every case below against float64 is 1.16e-7 on the emulator
# (forward, 40 003 rows; 1.08e-7 at L = 280 with or without the +-3000 shift -- the row maximum is subtracted exactly) and 1.36e-7 on an
# MI355X; _SOFTMAX_F32 = 4 x the larger, against test_softmax's 3e-5.  bf16 keeps test_softmax's bounds (one rounding of the output,
# 2^-8 of a row's maximum: 2.9e-3 forward and 3.6e-3 backward measured).
_SOFTMAX_F32 = 5.5e-7
_SOFTMAX_TOL = {_F32: (_SOFTMAX_F32, 0.0), _BF16: (1.6e-2, 2e-4)}


def _softmax_case(tgt, dt, s, alpha, name):
    rows, Lc = s.shape
    gen = torch.Generator().manual_seed(rows + Lc)
    s = s.to(dt)
    ref = torch.softmax(alpha * s.double(), -1)
    p = ops.softmax_fwd_(tgt.to(s.clone()), rows, Lc, alpha)
    tol, atol = _SOFTMAX_TOL[dt]
    assert bool(torch.isfinite(p.float()).all()), f'{name}: forward not finite'
    assert_close(p, ref, tol, name=f'softmax fwd [{name}]')
    pin = ref.to(dt)                      # the backward's input: the (peaked, shifted) probabilities in the kernel's storage type
    dp = torch.randn(rows, Lc, generator=gen).to(dt)
    dref = alpha * pin.double() * (dp.double() - (pin.double() * dp.double()).sum(-1, keepdim=True))
    ds = ops.softmax_bwd_(tgt.to(pin.clone()), tgt.to(dp.clone()), rows, Lc, alpha)
    assert_close(ds, dref, tol, atol=atol, name=f'softmax bwd [{name}]')
    print(f'softmax {name} {dt} [{tgt.kind}]: fwd {(p.double().cpu() - ref).abs().max().item() / ref.abs().max().item():.3g}, '
          f'bwd {(ds.double().cpu() - dref).abs().max().item() / max(dref.abs().max().item(), 1e-30):.3g} of max')


@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('L_', [1, 63, 64, 65, 1023, 1024])
def test_softmax_row_lengths(tgt, dt, L_):
    """19 rows of every length at which the per-lane loop changes: one element, one short of a wave, a wave, one over, and the last two
    the kernel supports"""
    s = torch.randn(19, L_, generator=torch.Generator().manual_seed(L_)) * 3
    _softmax_case(tgt, dt, s, 0.125, f'L={L_}')


@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
def test_softmax_grid_stride(tgt, dt):
    """40 003 rows of 24: more than the 8192 x 4 rows one sweep of the grid covers (stage 1 has B x 16 384 rows); rows 32 768 ... 40 002
    are only reached by the second trip of the loop, and 40 003 is not a multiple of the 4 rows per block"""
    s = torch.randn(40003, 24, generator=torch.Generator().manual_seed(7)) * 3
    _softmax_case(tgt, dt, s, 0.125, 'rows=40003')


@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('family', ['shift+3000', 'shift-3000', 'onehot'])
@pytest.mark.parametrize('L_', [24, 280])
def test_softmax_range(tgt, dt, L_, family):
    """alpha * s = +-375 + O(1): exp overflows (or is 0 / 0) unless the row maximum is subtracted; one-hot rows: one logit 60 above
    the rest, and the backward runs on those peaked probabilities"""
    s = torch.randn(19, L_, generator=torch.Generator().manual_seed(L_ + len(family))) * 3
    if family == 'onehot':
        s[torch.arange(19), torch.arange(19) * 5 % L_] += 60 / 0.125
    else:
        s = s + float(family[5:])
    _softmax_case(tgt, dt, s, 0.125, f'L={L_} {family}')


def test_softmax_refuses_rows_longer_than_1024(tgt):
    s = tgt.to(torch.zeros(3, 1025))
    with pytest.raises(L.CmdaError):
        ops.softmax_fwd_(s, 3, 1025, 0.125)
    with pytest.raises(L.CmdaError):
        ops.softmax_bwd_(s, tgt.to(torch.zeros(3, 1025)), 3, 1025, 0.125)


# ====================================================================================================================== LayerNorm
# x ~ N(mu, 1) per row with mu / sigma in {0, 10, 1000}, and N(0, 1) with one channel at 1e4 (an outlier channel of the fp32 residual
# stream).  A two-pass variance (centre, then square) does not depend on the ratio; the one-pass form E[x^2] - E[x]^2 loses
# (mu / sigma)^2: 1e6 x 2^-24 at ratio 1000.
#   variance, read back from the saved rstd: |var_k - var| / var <= _LN_VAR_K 2^-24.   Worst, emulator: 5.48 / 5.12 / 4.51 at the three
#      ratios, 7.67 with the outlier channel; MI355X: 4.02 / 3.87 / 4.55 and 6.69.
#   mean: |mean_k - mean| <= _LN_MEAN_K 2^-24 max(1, |mean|).   Worst, emulator and MI355X alike: 0.72 / 2.18 / 2.02 and 4.79.
#   y: the two above imply |dy| <= |gamma| (|dmean| rstd + |xhat| dvar / (2 var)), plus 4 roundings of the fp32 evaluation itself
#      (x - mean, * rstd, * gamma, + beta) on max |y|.  At ratio 1000 that is ~1e-4 absolute: the fp32 mean of numbers near 1000, not
#      a defect.
#   backward from the kernel's own statistics at ratio 1000: xhat carries delta = |dmean| rstd (ulp(1000) / sigma), the same for every
#      channel of a row, so with c1 = mean(gy), c2 = mean(gy xhat): |ddx| <= rstd delta (|c2| + |xhat| |c1|), |ddgamma| <= delta sum_rows |dy|.
_LN_VAR_K = 31.0
_LN_MEAN_K = 19.2
_LN_CASES = {'ratio0': (0.0, None), 'ratio10': (10.0, None), 'ratio1000': (1000.0, None), 'outlier_channel': (0.0, 1e4)}


def _ln_ref64(x, g, b, eps):
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    rs = (var + eps).rsqrt()
    xhat = (x64 - mu) * rs
    return mu, var, rs, xhat, xhat * g.double() + b.double()


def _ln_fwd(tgt, entry, x, g, b, eps):
    xd, gd, bd = tgt.to(x), tgt.to(g), tgt.to(b)
    rows, C = x.shape
    if entry == 'fwd2':
        return ops.layernorm_fwd(xd, gd, bd, eps)
    y, mean, rstd = torch.empty_like(xd), torch.empty(rows, device=tgt.device), torch.empty(rows, device=tgt.device)
    L.call('cmda_layernorm_fwd', L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(y), L.ptr(mean), L.ptr(rstd), L.c_i64(rows), L.c_i32(C),
           L.c_f32(eps), L.dtype_tag(xd), L.stream_of(xd))
    return y, mean, rstd


@pytest.mark.parametrize('entry', ['fwd', 'fwd2'])
@pytest.mark.parametrize('case', list(_LN_CASES))
@pytest.mark.parametrize('C', [32, 160, 320, 1024])
def test_layernorm_conditioning(tgt, C, case, entry):
    """fp32 x, 300 rows; C = 32: several rows per wave, 160: a ragged vector count, 320 / 1024: 2 (5 on 16 lanes) and 4 passes"""
    rows, eps = 300, 1e-6
    ratio, outlier = _LN_CASES[case]
    gen = torch.Generator().manual_seed(C + int(ratio))
    x = torch.randn(rows, C, generator=gen) + ratio
    if outlier is not None:
        x[:, C // 3] = outlier
    g, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    mu, var, rs, xhat, yref = _ln_ref64(x, g, b, eps)
    y, mean_k, rstd_k = _ln_fwd(tgt, entry, x, g, b, eps)
    var_k = rstd_k.double().cpu() ** -2 - eps
    mean_k = mean_k.double().cpu()
    rv = ((var_k - var[:, 0]).abs() / var[:, 0]).max().item() / _EPS24
    rm = ((mean_k - mu[:, 0]).abs() / mu[:, 0].abs().clamp(min=1.0)).max().item() / _EPS24
    print(f'ln conditioning C={C} {case} {entry} [{tgt.kind}]: var err / 2^-24 = {rv:.3f}, mean err / (2^-24 max(1, |mean|)) = {rm:.3f}, '
          f'y abs err {(y.double().cpu() - yref).abs().max().item():.3g}')
    check_le('ln variance: relative error / 2^-24', rv, _LN_VAR_K)
    check_le('ln mean: error / (2^-24 max(1, |mean|))', rm, _LN_MEAN_K)
    dmean = _LN_MEAN_K * _EPS24 * mu.abs().clamp(min=1.0)
    bound = (g.double().abs() * (dmean * rs + xhat.abs() * 0.5 * _LN_VAR_K * _EPS24)).max().item() + 4 * _EPS24 * yref.abs().max().item()
    check_le('ln y: absolute error against the bound the statistics imply', (y.double().cpu() - yref).abs().max().item(), bound)


@pytest.mark.parametrize('entry', ['bwd', 'bwd2'])
@pytest.mark.parametrize('C', [32, 160, 320, 1024])
def test_layernorm_backward_at_ratio_1000(tgt, C, entry):
    """dx, dgamma, dbeta from the kernel's OWN saved mean / rstd at mu / sigma = 1000 against float64; bwd: fp32 gradients through the
    one-dtype entry point, bwd2: bf16 gradients with the fp32 x (the residual-stream form)"""
    rows, eps = 300, 1e-6
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(rows, C, generator=gen) + 1000.0
    g, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    dy = torch.randn(rows, C, generator=gen)
    dt = _F32 if entry == 'bwd' else _BF16
    dy = dy.to(dt)
    mu, var, rs, xhat, _ = _ln_ref64(x, g, b, eps)
    gy = dy.double() * g.double()
    c1, c2 = gy.mean(1, keepdim=True), (gy * xhat).mean(1, keepdim=True)
    dxref = rs * (gy - c1 - xhat * c2)
    _, mean, rstd = _ln_fwd(tgt, 'fwd2', x, g, b, eps)
    xd, gd, dyd = tgt.to(x), tgt.to(g), tgt.to(dy)
    dg, db = torch.zeros(C, device=tgt.device), torch.zeros(C, device=tgt.device)
    if entry == 'bwd2':
        dx = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, dg, db)
    else:
        ws = torch.zeros(int(L.lib().cmda_layernorm_bwd_ws_floats(rows, C)), device=tgt.device)
        dx = torch.empty_like(dyd)
        L.call('cmda_layernorm_bwd', L.ptr(dyd), L.ptr(xd), L.ptr(gd), L.ptr(mean), L.ptr(rstd), None, L.ptr(dx), L.ptr(dg), L.ptr(db),
               L.ptr(ws), L.c_i64(rows), L.c_i32(C), None, L.c_i64(0), None, L.dtype_tag(xd), L.stream_of(xd))
        assert ws.abs().max().item() == 0.0, 'the workspace is zero again when the call completes'
    delta = _LN_MEAN_K * _EPS24 * mu.abs().clamp(min=1.0) * rs          # error of xhat: the fp32 mean of numbers near 1000
    tol = 3e-5 if dt == _F32 else 1.6e-2                                 # test_layernorm's bounds for well-conditioned rows
    dx_extra = (rs * delta * (c2.abs() + xhat.abs() * c1.abs())).max().item()
    assert_close(dx, dxref, tol, atol=dx_extra, name=f'ln dx at ratio 1000 ({entry})')
    dg_extra = (delta * dy.double().abs()).sum(0).max().item()
    assert_close(dg, (dy.double() * xhat).sum(0), 2e-5, atol=dg_extra, name=f'ln dgamma at ratio 1000 ({entry})')
    assert_close(db, dy.double().sum(0), 2e-5, name=f'ln dbeta at ratio 1000 ({entry})')


# ==================================================================================================== cross-entropy, pseudo-labels
# Float64 F.interpolate + F.cross_entropy.  Families: +-300 per image (the bilinear mix of a constant is that constant), one class
# +100 everywhere, a random class +60 per low-resolution pixel (lse, the argmax and the 0.968 threshold all move across pixels).
# Labels outside [0, nc) other than 255 -- 19 / 200 / -1 -- are skipped by the kernels and ignored by the reference, for the loss, the
# gradient and the `correct` count.  Sizes: (8, 12) -> (32, 48), the staged tile; (9, 70) -> (9, 70) with nc = 19, where a tile's patch
# is 65 * 9 * 19 = 11 115 floats > the 6144 of LDS and tile_scores reads global memory (nc = 7: 4095, staged); and (9, 70) -> (18, 70),
# unstaged too (65 * 6 * 19 = 7410) but with vertical weights 1/4 and 3/4 -- at the identity size three of the four taps have weight 0
# and a wrong tap address would go unseen.  All three have ratios whose fp32 source coordinates are exact (1, 2, 4), so the weights
# are: a ratio like 75 / 70 puts ulp(70) into every weight, 63 x 2^-24 max |logit| of lse here, which is the coordinate's rounding
# (torch's own fp32 interpolate has it, see test_upsample_logits_nchw) and would drown the term being measured.
# Bounds: loss 2e-6 and dlogits 2e-5 relative (test_ce_upsample's); lse absolute and the probabilities (pseudo-label, dlogits) get a
# term for the fp32 spacing of the logits themselves:
#   |lse_k - lse| <= _CE_LSE_K 2^-24 max(1, max |logit|):   worst ratio 2.26 on the emulator (3.6e-5 = ulp(300) under the shift), 2.26
#                                                           on an MI355X
#   |p_k - p| <= 1e-5 + _CE_PROB_K 2^-24 max |logit|:       worst err / (2^-24 max |logit|) 0.96 on the emulator (1.76e-5 under the shift,
#                                                           above test_pseudo_label's 1e-5, which was set for logits of order 4), 0.96
#                                                           on an MI355X
_CE_LSE_K = 9.1
_CE_PROB_K = 3.9
_CE_FAMILIES = ['randn', 'shift+300', 'shift-300', 'class+100', 'pixel_class+60']
_CE_SIZES = [(2, 8, 12, 32, 48), (1, 9, 70, 9, 70), (1, 9, 70, 18, 70)]


def _ce_logits(family, B, h, w, nc, gen):
    lg = torch.randn(B, h, w, nc, generator=gen) * 2
    if family.startswith('shift'):
        lg += float(family[5:]) * (1 - 2 * (torch.arange(B) % 2)).view(B, 1, 1, 1).float()   # per image: +, -, +, ...
    elif family == 'class+100':
        lg[..., nc // 2] += 100
    elif family == 'pixel_class+60':
        lg.scatter_add_(3, torch.randint(0, nc, (B, h, w, 1), generator=gen), torch.full((B, h, w, 1), 60.0))
    return lg


@pytest.mark.parametrize('use_weight', [True, False], ids=['weighted', 'unweighted'])
@pytest.mark.parametrize('nc', [19, 7])
@pytest.mark.parametrize('B,h,w,H,W', _CE_SIZES)
@pytest.mark.parametrize('family', _CE_FAMILIES)
def test_ce_upsample_range(tgt, family, B, h, w, H, W, nc, use_weight):
    gen = torch.Generator().manual_seed(h + nc + len(family))
    logits = _ce_logits(family, B, h, w, nc, gen)
    label = torch.randint(0, nc, (B, H, W), generator=gen)
    r = torch.rand(B, H, W, generator=gen)
    label[r < 0.1] = 255
    label[(r >= 0.1) & (r < 0.13)] = nc            # (19 for nc = 19: the first value past the classes)
    label[(r >= 0.13) & (r < 0.16)] = 200
    label[(r >= 0.16) & (r < 0.19)] = -1
    weight = torch.rand(B, H, W, generator=gen) if use_weight else None
    lab_ref = torch.where((label >= 0) & (label < nc), label, torch.full_like(label, 255))
    lr = logits.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(lr, size=(H, W), mode='bilinear', align_corners=False)
    loss_px = F.cross_entropy(up, lab_ref, reduction='none', ignore_index=255)
    if use_weight:
        loss_px = loss_px * weight.double()
    n = B * H * W
    loss = loss_px.sum() / n
    (loss * 0.7).backward()
    correct = int((up.argmax(1) == lab_ref).sum())
    acc, lse = ops.ce_upsample_fwd(tgt.to(logits), tgt.to(label), tgt.to(weight), H, W)
    _rel_le('ce loss', acc[0:1] / n, loss.detach().view(1), 2e-6)
    top2 = up.detach().topk(2, 1).values
    near_tie = int(((top2[:, 0] - top2[:, 1]) < 1e-5 * top2[:, 0].abs().clamp(min=1.0)).sum())
    check_le('ce correct count (beyond near ties of the argmax)', abs(acc[1].item() - correct), near_tie)
    amax = max(1.0, logits.abs().max().item())
    rl = (lse.double().cpu() - torch.logsumexp(up.detach(), 1)).abs().max().item() / (_EPS24 * amax)
    print(f'ce lse {family} {(B, h, w, H, W, nc)} [{tgt.kind}]: err / (2^-24 max |logit|) = {rl:.3f}')
    check_le('ce lse: absolute error / (2^-24 max |logit|)', rl, _CE_LSE_K)
    gs = tgt.to(torch.tensor([0.7]))
    dl = ops.ce_upsample_bwd(tgt.to(logits), tgt.to(label), tgt.to(weight), lse, gs, 1.0 / n, H, W)
    # dlogits = weight (softmax - onehot): a probability, so test_ce_upsample's 2e-5 gets the same term as the pseudo-label probability
    # (1.45e-5 of max measured under the +-300 shift at one image, 0.79 x 2^-24 max |logit|, emulator and MI355X alike)
    assert_close(dl, lr.grad.permute(0, 2, 3, 1), 2e-5 + _CE_PROB_K * _EPS24 * logits.abs().max().item(), name='ce dlogits')


@pytest.mark.parametrize('nc', [19, 7])
@pytest.mark.parametrize('B,h,w,H,W', _CE_SIZES)
@pytest.mark.parametrize('family', _CE_FAMILIES)
def test_pseudo_label_range(tgt, family, B, h, w, H, W, nc):
    gen = torch.Generator().manual_seed(h + nc + len(family) + 1)
    logits = _ce_logits(family, B, h, w, nc, gen)
    up = F.interpolate(logits.double().permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False)
    prob_ref, lab_ref = torch.softmax(up, 1).max(1)
    lab, prob, cnt = ops.pseudo_label(tgt.to(logits), H, W, 0.968)
    top2 = up.topk(2, 1).values
    near_tie = (top2[:, 0] - top2[:, 1]) < 1e-5 * top2[:, 0].abs().clamp(min=1.0)
    assert bool(((lab.cpu() == lab_ref) | near_tie).all()), 'pseudo-labels differ away from a near tie'
    amax = logits.abs().max().item()
    perr = (prob.double().cpu() - prob_ref).abs().max().item()
    print(f'pseudo prob {family} {(B, h, w, H, W, nc)} [{tgt.kind}]: err {perr:.3g}, err / (2^-24 max |logit|) = {perr / (_EPS24 * amax):.3f}')
    check_le('pseudo prob: absolute error', perr, 1e-5 + _CE_PROB_K * _EPS24 * amax)
    nref = int((prob_ref >= 0.968).sum())
    if family in ('class+100', 'pixel_class+60'):
        assert nref > 0.9 * B * H * W if family == 'class+100' else nref > 100, 'the case is meant to put many pixels over the threshold'
    check_le('pseudo count: |count - reference|', abs(cnt.item() - nref), 2)


@pytest.mark.parametrize('nc', [19, 7])
@pytest.mark.parametrize('family', ['shift+300', 'shift-300'])
def test_upsample_logits_range(tgt, family, nc):
    """the mix of four logits near +-300 is exact up to one rounding of the mix (the weights sum to 1 within an ulp): the bound of
    test_upsample_logits_nchw, 4e-6 of the largest element (= 20 ulp(300) here, against the 1 ... 2 expected), holds unchanged"""
    B, h, w, H, W = 2, 5, 7, 13, 18
    logits = _ce_logits(family, B, h, w, nc, torch.Generator().manual_seed(nc))
    ref = F.interpolate(logits.double().permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False)
    out = ops.upsample_logits_nchw(tgt.to(logits), H, W)
    assert_close(out, ref, 4e-6, name='upsample logits nchw (shifted)')


# ====================================================================================================================== GELU
# common.h evaluates erf by Abramowitz & Stegun 7.1.26 (|error| < 1.5e-7 in exact arithmetic).  z on a grid over [-12, 12] with +-0:
#   value       err / (0.5 |z| 1.5e-7 + 2^-24 |ref|): the series' bound through 0.5 z (1 + erf) plus one rounding of the result
#   derivative  err / (0.5 * 1.5e-7 + 2^-24 (|ref| + |z| pdf(z))): cdf + z pdf
# Worst ratios, fp32: value 1.96 on the emulator (4.4e-7 at z = 3.17: the fp32 evaluation of 1 - poly * e adds its own rounding) and
# 1.75 on an MI355X, derivative 1.83 (2.1e-7) and 1.83 (1.9e-7).  bf16 (the row-walking kernels) adds one rounding of the stored result,
# 2^-8 |ref|; what is left of its error after that is under 0.2 of the denominator.
_GELU_K = 7.9
_GELU_GRAD_K = 7.4
_GELU_SHAPE = (1, 5, 40, 24)   # 4800 points


def _gelu_grid(dt):
    n = math.prod(_GELU_SHAPE)
    z = torch.cat([torch.linspace(-12, 12, n - 2), torch.tensor([0.0, -0.0])]).to(dt)
    z64 = z.double()
    pdf = torch.exp(-0.5 * z64 * z64) / math.sqrt(2 * math.pi)
    cdf = 0.5 * (1 + torch.erf(z64 / math.sqrt(2)))
    return z, z64, z64 * cdf, cdf + z64 * pdf, pdf


def _gelu_check(name, got, ref, denom, k, tgt, rounding=0.0):
    """worst (|got - ref| - rounding |ref|) / denom under k; rounding: the storage format's own (bf16 outputs)"""
    got = got.double().cpu().flatten()
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    ratio = (((got - ref).abs() - rounding * ref.abs()).clamp(min=0) / denom).max().item()
    print(f'{name} [{tgt.kind}]: worst ratio {ratio:.3f}, worst abs err {(got - ref).abs().max().item():.3g}')
    check_le(name, ratio, k)


@pytest.mark.parametrize('dt', [_F32, _BF16], ids=['f32', 'bf16'])
def test_gelu_range_depthwise(tgt, dt):
    """dwconv_fwd(act='gelu') with a centre-tap-only weight and zero bias (fp32: the row-run kernels, bf16: the walk), and both
    backward preparations with dy = 1"""
    B, H, W, C = _GELU_SHAPE
    z, z64, val, grad, pdf = _gelu_grid(dt)
    rnd = 2.0 ** -8 if dt == _BF16 else 0.0   # (8 significant bits: half an ulp is at most 2^-8 of the value)
    w = torch.zeros(9, C)
    w[4] = 1.0
    xd, wd, bd = tgt.to(z.view(B, H, W, C)), tgt.to(w), tgt.to(torch.zeros(C))
    one = tgt.to(torch.ones(B, H, W, C).to(dt))
    y = ops.dwconv_fwd(xd, wd, bd, B, H, W, C, 1, 'gelu')
    dv = 0.5 * z64.abs() * 1.5e-7 + _EPS24 * val.abs() + 1e-38
    _gelu_check(f'gelu value (depthwise, {dt})', y, val, dv, _GELU_K, tgt, rnd)
    dd = 0.5 * 1.5e-7 + _EPS24 * (grad.abs() + z64.abs() * pdf)
    dz = ops.dwconv_gelu_bwd_prep(xd, wd, bd, one, B, H, W, C, 1)
    _gelu_check(f'gelu derivative (bwd_prep, {dt})', dz, grad, dd, _GELU_GRAD_K, tgt, rnd)
    dw, db = torch.zeros(C, 9, device=tgt.device), torch.zeros(C, device=tgt.device)
    dz2 = ops.dwconv_gelu_bwd_fused(xd, wd, bd, one, dw, db, B, H, W, C, 1)
    _gelu_check(f'gelu derivative (bwd_fused, {dt})', dz2, grad, dd, _GELU_GRAD_K, tgt, rnd)


def test_gelu_range_gemm_epilogue(tgt):
    """the GEMM act='gelu' epilogue on z @ I (fp32: every product with the identity is exact)"""
    z, z64, val, _, _ = _gelu_grid(_F32)
    M, N = z.numel() // 64, 64
    a, eye = tgt.to(z.view(M, N).contiguous()), tgt.to(torch.eye(N))
    out = torch.empty(M, N, device=tgt.device)
    ops.gemm(ops.plain_view(a, M, N), ops.plain_view(eye, N, N), out, M, N, N, dtype=0, act='gelu')
    dv = 0.5 * z64.abs() * 1.5e-7 + _EPS24 * val.abs() + 1e-38
    _gelu_check('gelu value (GEMM epilogue)', out, val, dv, _GELU_K, tgt)
