"""cmdax4_cow_mask / cmdax4_cow_field (cow_mask.hip): the cow-mask dropout of the source ISR.  The checker is an fp64 torch restatement
of cow_masks (datasets/utils.py:171-200) written here: reflect pad, two conv2d, std_mean; tests/golden/isr3.npz holds the
reference's own draws, field and mask for two seeds."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cmda_amd import _lib, ops
from conftest import check_le

HERE = os.path.dirname(os.path.abspath(__file__))
BAND = 1e-4          # |smooth - thr| <= BAND * std: pixels whose side of the threshold fp32 arithmetic may decide either way
BAND_SHARE = 5e-4    # at most 0.05 % of the pixels may lie in that band
SMOOTH_TOL = 2e-5    # the smooth field against fp64, in units of its std (5 x the reference's own fp32 distance, 3.9e-6)


def _gold():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', 'isr3.npz')).items()}


def restate(field, taps, tf):
    """fp64: field [B,H,W], taps [B,K], tf [B] -> (smooth [B,H,W], thr [B], std [B])"""
    field, taps, tf = field.double(), taps.double(), tf.double()
    B, K = taps.shape
    R = (K - 1) // 2
    smooth = []
    for b in range(B):
        n = F.pad(field[b][None, None], pad=(R, R, 0, 0), mode='reflect')
        s = F.conv2d(n, taps[b][None, None, None, :])
        s = F.pad(s, pad=(0, 0, R, R), mode='reflect')
        smooth.append(F.conv2d(s, taps[b][None, None, :, None])[0, 0])
    smooth = torch.stack(smooth)
    std, mean = torch.std_mean(smooth, [1, 2])
    return smooth, tf * std + mean, std


def check_against_restatement(name, isr, out, smooth, field, taps, tf, expect_mask=None):
    """the two criteria: the smooth field within SMOOTH_TOL * std of fp64; the mask equal to fp64's (and to `expect_mask`) outside the
    band around the threshold, the band holding at most BAND_SHARE of the pixels; out = isr * mask exactly, all channels alike"""
    ref_s, thr, std = restate(field.cpu(), taps.cpu(), tf.cpu())
    isr, out, smooth = isr.cpu(), out.cpu(), smooth.cpu()
    B, C = isr.shape[:2]
    for b in range(B):
        check_le(f'{name}[{b}] smooth vs fp64 / std', ((smooth[b].double() - ref_s[b]).abs().max() / std[b]).item(), SMOOTH_TOL)
        band = (ref_s[b] - thr[b]).abs() <= BAND * std[b]
        check_le(f'{name}[{b}] share of pixels in the threshold band', band.float().mean().item(), BAND_SHARE)
        got = (out[b] != 0) | (isr[b] == 0)          # where the kernel kept the pixel (isr has no zeros in these tests)
        ref_mask = ref_s[b] <= thr[b]
        for c in range(C):
            assert torch.equal(got[c][~band], ref_mask[~band]), f'{name}[{b}] channel {c}: mask differs from fp64 outside the band'
            assert torch.equal(out[b, c], isr[b, c] * got[c].float()), f'{name}[{b}] channel {c}: out is not isr * mask'
            assert torch.equal(got[c], got[0]), f'{name}[{b}]: channel {c} has another mask'
        if expect_mask is not None:
            assert torch.equal(got[0][~band], expect_mask[b].bool()[~band]), f'{name}[{b}]: mask differs from the reference outside the band'
        kept = got[0].float().mean().item()
        check_le(f'{name}[{b}] |kept share - 0.7|', abs(kept - 0.7), 0.12)


def _isr(B, C, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g) * 1.8 - 0.9
    return torch.where(x.abs() < 0.01, torch.full_like(x, 0.5), x)   # no zeros: out != 0 reads the mask back


def _draws(sigmas, p=0.7, max_sigma=16):
    return [dict(p=p, sigma=s, max_sigma=max_sigma) for s in sigmas]


def test_draw_cow_mask_consumes_the_generator_as_the_reference(tgt):
    g = _gold()
    for s in g['cow_seeds'].tolist():
        torch.manual_seed(s)
        d = ops.draw_cow_mask()
        nxt = torch.rand(1)
        assert d['p'] == g[f'cow{s}_p'].item() and d['sigma'] == g[f'cow{s}_sigma'].item(), 'p and sigma bit for bit'
        assert torch.equal(nxt, g[f'cow{s}_next_rand']), 'the generator is left where the reference leaves it'


@pytest.mark.parametrize('seed', [0, 1])
def test_cow_mask_reproduces_the_reference(tgt, seed):
    g = _gold()
    field = g[f'cow{seed}_field'][None].contiguous()
    H, W = field.shape[1:]
    assert (H, W) == (100, 132)
    taps, tf = ops.cow_mask_params([dict(p=g[f'cow{seed}_p'].item(), sigma=g[f'cow{seed}_sigma'].item(), max_sigma=16)])
    assert taps.shape == (1, 195)
    isr = _isr(1, 3, H, W, seed)
    out, smooth = ops.cow_mask(tgt.to(isr), tgt.to(taps), tgt.to(tf), field=tgt.to(field), debug=True)
    check_against_restatement(f'golden seed {seed}', isr, out, smooth, field, taps, tf, expect_mask=g[f'cow{seed}_mask'][None])


def test_cow_mask_last_legal_padding(tgt):
    """98 x 98 with K = 195: the padding is side - 1; one pixel less is refused"""
    g = torch.Generator().manual_seed(9)
    field = torch.randn(1, 98, 98, generator=g)
    taps, tf = ops.cow_mask_params(_draws([16.4]))
    isr = _isr(1, 1, 98, 98, 2)
    out, smooth = ops.cow_mask(tgt.to(isr), tgt.to(taps), tgt.to(tf), field=tgt.to(field), debug=True)
    check_against_restatement('98x98', isr, out, smooth, field, taps, tf)
    with pytest.raises(_lib.CmdaError):
        ops.cow_mask(tgt.to(_isr(1, 1, 97, 120)), tgt.to(taps), tgt.to(tf), field=tgt.to(torch.randn(1, 97, 120, generator=g)))
    assert _lib.lib().cmdax4_cow_mask_ws_bytes(1, 97, 120, 195) == 0


@pytest.mark.parametrize('shape', [(24, 40), (70, 33)])
@pytest.mark.parametrize('C', [1, 3])
def test_cow_mask_small_kernel(tgt, shape, C):
    """K = 9, three samples with three sigmas; gate, in place, run-to-run"""
    H, W = shape
    B = 3
    # (at 960 pixels one pixel in the threshold band is already 0.1 %: the seeds are ones whose fp64 restatement has none there --
    # a property of the inputs and the restatement alone, the condition check_against_restatement asserts before it looks at the kernel)
    g = torch.Generator().manual_seed(100 + H)
    field = torch.randn(B, H, W, generator=g)
    taps, tf = ops.cow_mask_params(_draws([0.8, 1.1, 1.3]), half_width=4)
    assert taps.shape == (B, 9)
    isr = _isr(B, C, H, W, 3)
    d = [tgt.to(t) for t in (isr, taps, tf, field)]
    out, smooth = ops.cow_mask(d[0], d[1], d[2], field=d[3], debug=True)
    check_against_restatement(f'K=9 {H}x{W} C={C}', isr, out, smooth, field, taps, tf)
    again = ops.cow_mask(d[0], d[1], d[2], field=d[3])
    assert torch.equal(again.cpu(), out.cpu()), 'two runs are bit-identical'
    gate = tgt.to(torch.tensor([1, 0, 1], dtype=torch.int32))
    gated = ops.cow_mask(d[0], d[1], d[2], field=d[3], enable=gate).cpu()
    assert torch.equal(gated[1], isr[1]), 'a gated sample is its input bit for bit'
    assert torch.equal(gated[0], out.cpu()[0]) and torch.equal(gated[2], out.cpu()[2])
    buf = d[0].clone()
    assert ops.cow_mask(buf, d[1], d[2], field=d[3], out=buf) is buf
    assert torch.equal(buf.cpu(), out.cpu()), 'in place equals out of place'


def test_cow_mask_generated_field(tgt):
    B, H, W = 2, 40, 52
    taps, tf = (tgt.to(t) for t in ops.cow_mask_params(_draws([1.0, 1.2]), half_width=4))
    isr = tgt.to(_isr(B, 3, H, W))
    seed, offset = 1234567, 5
    field = ops.cow_field(B, H, W, seed, offset, device=tgt.device)
    ref = ops.cow_mask(isr, taps, tf, field=field).cpu()
    assert torch.equal(ops.cow_mask(isr, taps, tf, seed=seed, offset=offset).cpu(), ref)
    od = tgt.to(torch.tensor([3], dtype=torch.int64))
    assert torch.equal(ops.cow_mask(isr, taps, tf, seed=seed, offset=2, offset_dev=od).cpu(), ref)
    assert torch.equal(ops.cow_field(B, H, W, seed, 2, offset_dev=od).cpu(), field.cpu())
    assert not torch.equal(ops.cow_mask(isr, taps, tf, seed=seed, offset=offset + 1).cpu(), ref)


def test_cow_field_statistics(tgt):
    """the five-sigma bounds of test_randn_fields_statistics, and independence of the ISR-noise fields of the same (seed, offset)"""
    B, H, W = 2, 128, 128
    N = H * W
    f = ops.cow_field(B, H, W, 99, 7, device=tgt.device).cpu().double()
    others = ops.randn_fields(B, H, W, 99, 7, device=tgt.device).cpu().double()
    assert torch.isfinite(f).all()
    for b in range(B):
        x = f[b].flatten()
        check_le(f'cow field [{b}] |mean|', x.mean().abs().item(), 5 / math.sqrt(N))
        check_le(f'cow field [{b}] |var - 1|', abs(x.var().item() - 1), 5 * math.sqrt(2 / N))
        p1 = math.erf(1 / math.sqrt(2))
        check_le(f'cow field [{b}] |share(|n| < 1) - erf|', abs((x.abs() < 1).double().mean().item() - p1), 5 * math.sqrt(p1 * (1 - p1) / N))
        for k in range(3):
            check_le(f'cow field [{b}] |corr with noise field {k}|', (x * others[k, b].flatten()).mean().abs().item(), 5 / math.sqrt(N))
    check_le('cow field |corr between samples|', (f[0].flatten() * f[1].flatten()).mean().abs().item(), 5 / math.sqrt(N))


def test_cow_mask_refusals(tgt):
    from cmda_amd._lib import c_i32, c_i64, ptr
    B, C, H, W, K = 2, 3, 24, 40, 9
    isr = tgt.to(_isr(B, C, H, W))
    sentinel = 7.0
    out = tgt.to(torch.full((B, C, H, W), sentinel))
    taps = tgt.to(torch.ones(B, 255))
    tf = tgt.to(torch.zeros(B))
    lib = _lib.lib()
    ws = tgt.to(torch.empty(lib.cmdax4_cow_mask_ws_bytes(B, H, W, K) // 8, dtype=torch.float64))

    def run(K_=K, H_=H, W_=W, C_=C, isr_=isr, out_=out, taps_=taps, tf_=tf, ws_=ws):
        return lib.cmdax4_cow_mask(ptr(isr_), ptr(out_), ptr(taps_), ptr(tf_), None, None, None, ptr(ws_), c_i32(B), c_i32(C_), c_i32(H_),
                                   c_i32(W_), c_i32(K_), ctypes.c_uint64(1), c_i64(0), None, _lib.stream_of(isr))
    SHAPE, UNSUP = -1, -4
    assert run(K_=8) == SHAPE and run(K_=0) == SHAPE, 'an even K'
    assert run(K_=257) == SHAPE, 'K > 255'
    assert run(K_=49) == SHAPE, '(K - 1) / 2 = 24 >= min(H, W)'
    assert run(C_=0) == SHAPE and run(H_=0) == SHAPE
    assert run(out_=None) == UNSUP and run(isr_=None) == UNSUP and run(taps_=None) == UNSUP and run(tf_=None) == UNSUP and run(ws_=None) == UNSUP
    assert lib.cmdax4_cow_field(None, c_i32(B), c_i32(H), c_i32(W), ctypes.c_uint64(1), c_i64(0), None, _lib.stream_of(isr)) == UNSUP
    assert lib.cmdax4_cow_field(ptr(out), c_i32(B), c_i32(0), c_i32(W), ctypes.c_uint64(1), c_i64(0), None, _lib.stream_of(isr)) == SHAPE
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((B, C, H, W), sentinel)), 'a refused call writes nothing'
    with pytest.raises(_lib.CmdaError):
        ops.cow_mask(isr, tgt.to(torch.ones(B, 8)), tf, out=out)
    assert torch.equal(out.cpu(), torch.full((B, C, H, W), sentinel))
