"""The full-key instances of the fused attention kernels (attn_fwd_kernel<256, true>, attn_bwd_dq_kernel<true>): 256 live keys, head
dim 64, bf16, scale > 0 -- no key mask, the scale folded into an exp2, unnormalised probabilities into the second GEMM and 1 / l on
the outputs.  Every other key count (and scale <= 0) stays on the masked kernels, which these tests use as the second reference.

Reference: the float64 restatement of test_kernels.py::_attention_ref and its autograd on the same bf16 inputs.
Bounds: the suite's own from test_kernels.py::test_fused_attention, relative to the maximum of each output: 1.6e-2 for o, 2e-2 for
dq, dk, dv.  Measured maxima of these very cases on the commit before the full-key instances and with them, emulator and MI355X:
profiles/attn_fullkeys_errors.txt."""
import functools

import pytest
import torch

from cmda_amd import ops
from conftest import check_le

_BF16 = torch.bfloat16
_TOL_O, _TOL_G = 1.6e-2, 2e-2
_SCALE = 0.125


def _ref64(q, kv, do, B, N, Nk, heads, scale):
    """o, dq, dk, dv in float64 (mix_transformer.py:97-101 and its autograd)"""
    C = heads * 64
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qf = qr.view(B, N, heads, 64).permute(0, 2, 1, 3)
    k = kvr[:, :C].reshape(B, Nk, heads, 64).permute(0, 2, 1, 3)
    v = kvr[:, C:].reshape(B, Nk, heads, 64).permute(0, 2, 1, 3)
    a = (qf @ k.transpose(-1, -2) * scale).softmax(-1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(B * N, C)
    o.backward(do.double())
    return dict(o=o.detach(), dq=qr.grad, dk=kvr.grad[:, :C].clone(), dv=kvr.grad[:, C:].clone())


@functools.lru_cache(maxsize=None)
def _problem(kind, B, N, Nk, heads, scale=_SCALE):
    """bf16 q, kv, do and the float64 reference; computed once per case and shared by the emulator and the GPU run.
    kind: 'randn' | 'x4' (q scaled by 4) | 'fold' (q scaled by 8: scaled logits of std 8, rows near one-hot; queries 32 ... 47 of every
    batch exactly zero: uniform rows at 1 / 256) | ('keys', n): the first n of 256 key rows per batch of the 'randn' draw at 256 keys"""
    C = heads * 64
    if isinstance(kind, tuple):
        q, kv, do, _ = _problem('randn', B, N, 256, heads, scale)
        kv = kv.view(B, 256, 2 * C)[:, :Nk].reshape(B * Nk, 2 * C).contiguous()
    else:
        g = torch.Generator().manual_seed(1000 * N + 10 * heads + B)
        q, kv, do = (torch.randn(r, c, generator=g).to(_BF16) for r, c in ((B * N, C), (B * Nk, 2 * C), (B * N, C)))
        if kind == 'x4':
            q = q * 4
        elif kind == 'fold':
            q = q * 8
            q.view(B, N, C)[:, 32:48] = 0
    return q, kv, do, _ref64(q, kv, do, B, N, Nk, heads, scale)


def _rel_le(name, got, ref, tol, scale=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    scale = max(ref.abs().max().item() if scale is None else scale, 1e-30)
    err = (got - ref).abs().max().item() / scale
    print(f'{name}: {err:.3e} (bound {tol:.1e})')
    check_le(name, err, tol)


def _run(tgt, q, kv, do, B, N, Nk, heads, scale=_SCALE, direct=True):
    """o, dq, dk, dv of the accumulating form (fp32 workspace) and, with `direct`, dq, dk, dv of the direct form (bf16, N <= 1024)"""
    C = heads * 64
    qd, kvd, dod = tgt.to(q), tgt.to(kv), tgt.to(do)
    assert ops.attention_fused_ok(qd, Nk, heads, C)
    out = dict(o=ops.attention_fused_fwd(qd, kvd, B, N, Nk, heads, C, scale))
    dkv = torch.zeros(B * Nk, 2 * C, device=tgt.device)
    out['dq'] = ops.attention_fused_bwd(qd, kvd, dod, dkv, B, N, Nk, heads, C, scale)
    out['dk'], out['dv'] = dkv[:, :C], dkv[:, C:]
    if direct:
        assert ops.attention_bwd_direct(B, N, Nk, heads)
        dkv16 = torch.full((B * Nk, 2 * C), float('nan'), dtype=_BF16, device=tgt.device)   # NaN on entry: every element is written
        out['dq (direct)'] = ops.attention_fused_bwd(qd, kvd, dod, None, B, N, Nk, heads, C, scale, dkv16=dkv16)
        out['dk (direct)'], out['dv (direct)'] = dkv16[:, :C], dkv16[:, C:]
    return out


def _check(tag, out, ref, names=None):
    for name, got in out.items():
        base = name.split(' ')[0]
        if names is None or base in names:
            _rel_le(f'{tag} {name}', got, ref[base], _TOL_O if base == 'o' else _TOL_G)


@pytest.mark.parametrize('B,N,heads', [(1, 70, 1), (2, 200, 2)])
def test_fullkeys_ragged_rows(tgt, B, N, heads):
    """a partly filled last wave (70 = 64 + 6, 200 = 3 * 64 + 8): rows past N are clamped in load_qfrag and never stored"""
    q, kv, do, ref = _problem('randn', B, N, 256, heads)
    _check(f'full-key attention {(B, N, heads)}', _run(tgt, q, kv, do, B, N, 256, heads), ref)


@pytest.mark.parametrize('B', [32, 64])
def test_fullkeys_two_pass_blocks(tgt, B):
    """128 queries per block (two passes over 64, K / V loaded once): the full-key instances take it from 512 blocks of 128 up (the masked
    ones from 1024).  (32, 129, 8): 2 * 8 * 32 = 512 blocks, the second block of each pair holds one live row; one batch fewer stays at
    64 per block, and so does the same shape at 255 keys.  (64, 129, 8): 1024 blocks, the switch of the masked kernels"""
    N, heads = 129, 8
    assert ops.attention_fwd_queries_per_block(B, N, heads) == 128 and ops.attention_fwd_queries_per_block(31, N, heads) == 64
    assert ops.attention_fwd_queries_per_block(63, N, heads, Nk=255) == 64 and ops.attention_fwd_queries_per_block(64, N, heads, Nk=255) == 128
    assert ops.attention_fwd_queries_per_block(64, N, heads, scale=-0.125) == 128 and ops.attention_fwd_queries_per_block(63, N, heads, scale=0.0) == 64
    q, kv, do, ref = _problem('randn', B, N, 256, heads)
    _check(f'full-key attention, 128 queries per block, B = {B}', _run(tgt, q, kv, do, B, N, 256, heads, direct=False), ref)


_BOUNDARY = (1, 70, 2)


@pytest.mark.parametrize('Nk', [240, 255, 256])
def test_fullkeys_dispatch_boundary(tgt, Nk):
    """240 and 255 keys take the masked kernels, 256 the full-key ones; one draw, the first Nk key rows of it"""
    B, N, heads = _BOUNDARY
    q, kv, do, ref = _problem(('keys', Nk), B, N, Nk, heads)
    _check(f'attention at the dispatch boundary, {Nk} keys', _run(tgt, q, kv, do, B, N, Nk, heads), ref)


def test_fullkeys_against_masked_padded(tgt):
    """the masked kernels on 255 keys against the full-key kernels on the same data padded to 256 keys with a key that no query
    attends to: q[:, 0] = 8 in every head and the 256th key = (-128, 0, ..., 0), a scaled logit of -128 (the others are O(1)), so its
    probability is below e^-120 and its value row (1000) would show in o at once.  A wrong key row in the last tile fails here."""
    B, N, heads = _BOUNDARY
    C = heads * 64
    q, kv, do, _ = _problem(('keys', 255), B, N, 255, heads)
    q = q.clone()
    q[:, ::64] = 8
    masked = _run(tgt, q, kv, do, B, N, 255, heads)
    pad = torch.zeros(B, 1, 2 * C, dtype=_BF16)
    pad[:, :, 0:C:64] = -128
    pad[:, :, C:] = 1000
    kvp = torch.cat([kv.view(B, 255, 2 * C), pad], 1).reshape(B * 256, 2 * C).contiguous()
    full = _run(tgt, q, kvp, do, B, N, 256, heads)
    for name, got in full.items():
        base = name.split(' ')[0]
        want = masked[name].float().cpu()
        got = got.float().cpu()
        if base in ('dk', 'dv'):
            got = got.view(B, 256, C)
            last, got = got[:, 255], got[:, :255].reshape(B * 255, C)
            _rel_le(f'full-key on padded keys, {name} of the padding key (~0)', last, torch.zeros_like(last), _TOL_G,
                    scale=want.abs().max().item())
        _rel_le(f'full-key on padded keys vs masked on 255, {name}', got, want, _TOL_O if base == 'o' else _TOL_G)


def test_fullkeys_exponent_fold(tgt):
    """q scaled by 8: scaled logits of std 8 (maxima of several tens), rows near one-hot -- exp2(s c - m c) with the max over the raw
    scores; queries 32 ... 47 exactly zero: uniform rows, every exponential 1 and l = 256"""
    B, N, heads = 1, 70, 2
    q, kv, do, ref = _problem('fold', B, N, 256, heads)
    out = _run(tgt, q, kv, do, B, N, 256, heads)
    for name, got in out.items():
        assert bool(torch.isfinite(got.float()).all()), f'{name}: not finite'
    _check('full-key attention, exponent fold', out, ref, names=('o', 'dq'))
    z = slice(32, 48)
    _rel_le('full-key attention, uniform rows o', out['o'][z], ref['o'][z], _TOL_O, scale=ref['o'].abs().max().item())
    _rel_le('full-key attention, uniform rows dq', out['dq'][z], ref['dq'][z], _TOL_G, scale=ref['dq'].abs().max().item())


@pytest.mark.parametrize('B,N,heads', [(1, 260, 3), (1, 520, 1)])
def test_fullkeys_stats_contract(tgt, B, N, heads):
    """stats[b, h, q, 2] = (natural-log lse of the scaled scores, D) as the unchanged dK | dV kernels read them: accumulating form (fp32
    workspace; 4 waves) and direct form (bf16; 4 waves at 260 queries, 8 waves at 520), after the full-key dQ kernel.  q scaled by 4:
    lse spans tens, so an lse in the wrong base or of the unscaled scores moves every probability the second kernel rebuilds"""
    q, kv, do, ref = _problem('x4', B, N, 256, heads)
    _check(f'full-key attention, stats contract {(B, N, heads)}', _run(tgt, q, kv, do, B, N, 256, heads), ref)


@pytest.mark.parametrize('scale', [-0.125, 0.0])
def test_fullkeys_nonpositive_scale(tgt, scale):
    """scale <= 0 at 256 keys is served, by the masked kernels (the full-key ones take the max over the raw scores, which needs
    scale > 0).  scale = 0: uniform rows, dq and dk exactly zero"""
    B, N, heads = 1, 70, 1
    q, kv, do, ref = _problem('randn', B, N, 256, heads, scale)
    _check(f'attention at 256 keys, scale {scale}', _run(tgt, q, kv, do, B, N, 256, heads, scale=scale), ref)
