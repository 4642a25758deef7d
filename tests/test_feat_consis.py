"""Feature-consistency loss of the `isr_no_fusion` route (include/cmda_hip_ext9.h, the kernel in feat_dist.hip; reference:
encoder_decoder.py:833-848): `ops.feat_consis` on the emulator build and on the GPU against float64 written out here from the stored
(widened) inputs.

Bounds (the project's own): loss and level_loss 1e-5 relative (tests/test_fdist.py); the ADDED gradient 1e-5 of its maximum where the
block is fp32; a bf16 block 4e-3 of its maximum (one rounding of the sum, tests/test_resblock.py).  Starting gradients have the added
gradient's own magnitude, so the added part stays visible in the block's precision."""
import pytest
import torch

from cmda_amd import ops
from cmda_amd._lib import CmdaError
from conftest import check_le

MULTI = [(1024, 64), (256, 128), (64, 320), (15, 512)]
SHAPES = {
    '1x4': [(1, 4)],
    '3x20': [(3, 20)],            # 40-byte bf16 rows: no 16-byte alignment; 80-byte fp32 rows keep it
    '15x64': [(15, 64)],
    '515x320': [(515, 320)],
    '4099x512': [(4099, 512)],    # 257 fp32 chunks on 256 workgroups: one of them walks two chunks
    '8200x512': [(8200, 512)],    # the same in bf16 (257 chunks of 2048 sixteen-byte pieces)
    'four_levels': MULTI,
    'hundredfold': [(800, 64), (64, 8)],   # the first level 100 times the last
}
DTYPES = {'f32': (torch.float32, torch.float32), 'bf16': (torch.bfloat16, torch.bfloat16), 'bf16_f32grad': (torch.bfloat16, torch.float32)}
LAM, GSCALE = 0.4, 0.37


def _block(t, pad, fill, seed):
    """t as the middle columns of a wider buffer (pad columns of `fill`-scaled noise on either side): (buffer, view)"""
    if not pad:
        return t, t
    R, C = t.shape
    buf = (fill * torch.randn(R, C + 2 * pad, generator=torch.Generator().manual_seed(seed))).to(t.dtype)
    buf[:, pad:pad + C] = t
    return buf, buf[:, pad:pad + C]


def _inputs(shapes, fdt, gdt, pad=0, zero_grad=False, seed=3):
    g = torch.Generator().manual_seed(seed)
    lv = []
    for k, (R, C) in enumerate(shapes):
        a = (torch.randn(R, C, generator=g) + 0.5).to(fdt)
        b = torch.randn(R, C, generator=g).to(fdt)
        g0 = torch.zeros(R, C) if zero_grad else LAM * 2.0 / (R * C) * torch.randn(R, C, generator=g)
        # the pad differs per tensor, so the three row strides differ too
        lv.append(dict(a=_block(a, pad, 1.0, 10 + k), b=_block(b, pad and pad + 8, 1.0, 20 + k),
                       g=_block(g0.to(gdt), pad and pad + 16, LAM * 2.0 / (R * C), 30 + k)))
    return lv


def _reference(lv, gscale):
    """float64: (loss, level_loss, the added gradient per level)"""
    level, added = [], []
    for d in lv:
        a, b = d['a'][1].double(), d['b'][1].double()
        n = a.numel()
        diff = a - b
        level.append(LAM * (diff * diff).sum() / n)
        added.append(gscale * LAM * (2.0 / n) * diff)
    level = torch.stack(level)
    return level.sum(), level, added


def _run(tgt, lv, mode, gscale):
    """one call on fresh device copies of the inputs: (loss, level_loss, gradient buffers back on the host, ticket)"""
    dev = {k: [tgt.to(d[k][0].clone()) for d in lv] for k in 'abg'}
    view = lambda buf, d, k: buf if d[k][0] is d[k][1] else buf[:, d[k][1].storage_offset():d[k][1].storage_offset() + d[k][1].shape[1]]
    A = [view(t, d, 'a') for t, d in zip(dev['a'], lv)]
    B = [view(t, d, 'b') for t, d in zip(dev['b'], lv)]
    G = [view(t, d, 'g') for t, d in zip(dev['g'], lv)]
    gs = tgt.to(torch.tensor([gscale], dtype=torch.float32)) if gscale is not None else None
    loss, level = ops.feat_consis(A, B, LAM, gscale=gs, grads=None if mode == 'loss' else G, want_loss=mode != 'grad')
    ticket = int(ops._fd_ticket(A[0].device, 2).cpu())
    for t, d in zip(dev['a'] + dev['b'], [d['a'] for d in lv] + [d['b'] for d in lv]):
        assert torch.equal(t.cpu(), d[0]), 'a feature buffer was written'
    return (loss.cpu() if loss is not None else None, level.cpu() if level is not None else None, [t.cpu() for t in dev['g']], ticket)


def _check(tgt, lv, mode, gscale, gdt, name):
    ref_loss, ref_level, ref_added = _reference(lv, 1.0 if gscale is None else gscale)
    first = _run(tgt, lv, mode, gscale)
    again = _run(tgt, lv, mode, gscale)
    for out in (first, again):
        assert out[3] == 0, f'{name}: the ticket reads {out[3]} after the call'
    loss, level, bufs, _ = first
    if mode != 'grad':
        assert torch.equal(loss, again[0]) and torch.equal(level, again[1]), f'{name}: two calls differ in the loss'
        check_le(f'{name} loss rel err', abs(loss.double().item() - ref_loss.item()) / ref_loss.item(), 1e-5)
        check_le(f'{name} level_loss rel err (worst level)', ((level.double() - ref_level).abs() / ref_level).max().item(), 1e-5)
        # loss[0] is the sum of the level values in level order, in fp32
        s = torch.zeros((), dtype=torch.float32)
        for v in level:
            s = s + v
        assert loss.item() == s.item(), f'{name}: loss is not the in-order fp32 sum of level_loss'
    else:
        assert loss is None and level is None
    for k, (d, buf, buf2, add) in enumerate(zip(lv, bufs, again[2], ref_added)):
        assert torch.equal(buf, buf2), f'{name}: two calls differ in the gradient of level {k}'
        buf0, g0 = d['g']
        if mode == 'loss':
            assert torch.equal(buf, buf0), f'{name}: loss-only call wrote the gradient buffer of level {k}'
            continue
        off, C = (g0.storage_offset(), g0.shape[1]) if buf0 is not g0 else (0, g0.shape[1])
        got = buf[:, off:off + C].double()
        if buf0 is not g0:
            keep = torch.ones(buf0.shape[1], dtype=torch.bool)
            keep[off:off + C] = False
            assert torch.equal(buf[:, keep], buf0[:, keep]), f'{name}: columns next to the gradient block of level {k} changed'
        if gdt == torch.float32:
            err = ((got - g0.double()) - add).abs().max().item() / add.abs().max().item()
            check_le(f'{name} added gradient of level {k}, rel to its max', err, 1e-5)
        else:
            want = g0.double() + add
            check_le(f'{name} bf16 gradient block of level {k}, rel to its max', (got - want).abs().max().item() / want.abs().max().item(), 4e-3)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_feat_consis_against_float64(tgt, shape, dt):
    """loss and gradient in one launch, non-zero starting gradients (ADD semantics), gscale = 0.37; two calls bit-identical"""
    fdt, gdt = DTYPES[dt]
    _check(tgt, _inputs(SHAPES[shape], fdt, gdt), 'both', GSCALE, gdt, f'{shape} {dt}')


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('mode', ['loss', 'grad', 'both'])
@pytest.mark.parametrize('shape', ['515x320', 'four_levels'])
def test_feat_consis_modes(tgt, shape, mode, dt):
    """the three modes of the one kernel, one level and four; no gscale (1)"""
    fdt, gdt = DTYPES[dt]
    _check(tgt, _inputs(SHAPES[shape], fdt, gdt, zero_grad=mode == 'both'), mode, None, gdt, f'{shape} {mode} {dt}')


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('pad', [8, 3])
@pytest.mark.parametrize('shape', ['3x20', '515x320', 'four_levels'])
def test_feat_consis_strided_blocks(tgt, shape, pad, dt):
    """feature and gradient blocks as row-strided column slices of wider buffers (three different row strides; pad 8 keeps the
    16-byte alignment, pad 3 breaks it): the neighbouring columns come back untouched"""
    fdt, gdt = DTYPES[dt]
    _check(tgt, _inputs(SHAPES[shape], fdt, gdt, pad=pad), 'both', GSCALE, gdt, f'{shape} pad {pad} {dt}')


def test_feat_consis_some_levels_without_gradient(tgt):
    """a level whose gradient entry is None only contributes to the loss"""
    lv = _inputs(MULTI, torch.float32, torch.float32)
    A, B = [tgt.to(d['a'][0]) for d in lv], [tgt.to(d['b'][0]) for d in lv]
    G = [tgt.to(d['g'][0].clone()) if k % 2 == 0 else None for k, d in enumerate(lv)]
    loss, level = ops.feat_consis(A, B, LAM, grads=G)
    ref_loss, ref_level, ref_added = _reference(lv, 1.0)
    check_le('loss rel err', abs(loss.cpu().double().item() - ref_loss.item()) / ref_loss.item(), 1e-5)
    for k in (0, 2):
        err = ((G[k].cpu().double() - lv[k]['g'][0].double()) - ref_added[k]).abs().max().item() / ref_added[k].abs().max().item()
        check_le(f'added gradient of level {k}, rel to its max', err, 1e-5)


def test_feat_consis_refusals(tgt):
    a = tgt.to(torch.zeros(4, 8))
    with pytest.raises(CmdaError):
        ops.feat_consis([a], [a], LAM, want_loss=False)                       # nothing asked for
    with pytest.raises(CmdaError):
        ops.feat_consis([a] * 5, [a] * 5, LAM)                                # five levels
    with pytest.raises(CmdaError):
        ops.feat_consis([a], [a], LAM, grads=[tgt.to(torch.zeros(4, 8, dtype=torch.bfloat16))])   # bf16 gradient under fp32 features
