"""cmdax4_isr_multi (isr_multi.hip): C ISR channels of one gray map in one call, with an output window.  Checked against the
reference's own three-channel loop (tests/golden/isr3.npz) and, bit for bit, against the one-parameter entry point."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cmda_amd import _lib, ops
from cmda_amd.datasets import ISR3_PRESETS
from conftest import assert_close
from oracle import uda as ouda

HERE = os.path.dirname(os.path.abspath(__file__))
DIRECTIONS = ('rightdown', 'rightup', 'leftdown', 'leftup', 'all')
# three rows under one value range: shifts 1 / 3 / 5, a zero threshold among them
ROWS = [(0.0, 0.015, 1), (0.012, 0.12, 3), (0.025, 0.2, 5)]
VAL_RANGE = (9, 255 + 9)


def _gold():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', 'isr3.npz')).items()}


def _gray(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (B, H // 4 + 1, W // 4 + 1), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W]
    return (base * 0.8 + torch.randint(0, 52, (B, H, W), generator=g)).to(torch.uint8).contiguous()


def _rows(preset):
    return [(p['_threshold'], p['_clip_range'], p['shift_pixel']) for p in preset], preset[0]['val_range']


def test_isr_multi_reproduces_the_reference_presets(tgt):
    g = _gold()
    mean = torch.tensor(ouda.IMG_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(ouda.IMG_STD).view(1, 3, 1, 1)
    x = ((g['rgb'].permute(2, 0, 1)[None].float() + 0.5) - mean) / std
    gray = ops.isr_gray(tgt.to(x.contiguous()))
    assert torch.equal(gray.cpu()[0], torch.from_numpy(ouda.pil_luma(g['rgb'].numpy())))
    for name, preset in ISR3_PRESETS.items():
        rows, vr = _rows(preset)
        out = ops.isr_multi(gray, vr, ops.isr_multi_params(rows, 'rightdown', tgt.device, val_range=vr), 3).cpu()
        assert out.shape == (1, 3, 48, 72)
        for c in range(3):
            assert_close(out[0, c], g[f'isr_{name}'][c], 2e-6, atol=2e-7, name=f'isr3 {name} channel {c}')
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert not torch.equal(out[0, a], out[0, b]), f'{name}: channels {a} and {b} coincide'
        # the dict spelling builds the same table
        assert torch.equal(ops.isr_multi_params(preset, 'rightdown', tgt.device).cpu(),
                           ops.isr_multi_params(rows, 'rightdown', tgt.device, val_range=vr).cpu())


@pytest.mark.parametrize('shape', [(7, 9), (33, 70), (48, 72)])
@pytest.mark.parametrize('C', [1, 3])
def test_isr_multi_is_bit_identical_to_isr_from_gray(tgt, shape, C):
    H, W = shape
    gray = tgt.to(_gray(3, H, W, seed=H))
    for d in DIRECTIONS:
        prm = ops.isr_multi_params(ROWS[:C], d, tgt.device, val_range=VAL_RANGE)
        out = ops.isr_multi(gray, VAL_RANGE, prm, C, ndir_host=[4 if d == 'all' else 2] * C)
        assert out.shape == (3, C, H, W)
        for c in range(C):
            thr, clip, shift = ROWS[c]
            one = ops.isr_from_gray(gray, VAL_RANGE, thr, clip, shift, d)
            assert torch.equal(out[:, c].cpu(), one[:, 0].cpu()), f'{H}x{W} {d} channel {c}'


def test_isr_multi_flat_image(tgt):
    gray = tgt.to(torch.full((2, 20, 30), 77, dtype=torch.uint8))
    out = ops.isr_multi(gray, VAL_RANGE, ops.isr_multi_params(ROWS, 'rightdown', tgt.device, val_range=VAL_RANGE), 3).cpu()
    assert torch.isfinite(out).all()
    for c, (thr, clip, shift) in enumerate(ROWS):
        ref = ouda.image_change(gray[0].cpu().numpy(), shift, VAL_RANGE, thr, clip)
        assert_close(out[0, c:c + 1], ref, 2e-6, atol=2e-7, name=f'flat channel {c}')


def test_isr_multi_window(tgt):
    H, W, OH, OW = 40, 56, 17, 24
    # gray levels 100..200 (log differences up to 0.65, below every clip range of `rows`: 1.69 and more) except a black and a white
    # block in the bottom-right corner, whose borders carry the extreme differences of both signs (clipped: 1.69 ...), outside every
    # window below: a normalisation over the window alone gives other values
    rows = [(0.0, 0.5, 1), (0.0, 0.6, 3), (0.001, 0.7, 5)]
    gray = (100 + (_gray(3, H, W, seed=5).int() * 100) // 255).to(torch.uint8)
    gray[:, 34:, 46:] = 0
    gray[:, 37:, 51:] = 255
    gray = tgt.to(gray.contiguous())
    prm = ops.isr_multi_params(rows, 'rightdown', tgt.device, val_range=VAL_RANGE)
    full = ops.isr_multi(gray, VAL_RANGE, prm, 3).cpu()
    for wins in ([(3, 5, 0), (4, 2, 1), (11, 9, 1)], [(0, 0, 1), (W - OW - 14, H - OH - 8, 0), (7, 14, 0)]):
        win = tgt.to(torch.tensor(wins, dtype=torch.int32))
        out = ops.isr_multi(gray, VAL_RANGE, prm, 3, window=win, out_size=(OH, OW), window_host=wins).cpu()
        assert out.shape == (3, 3, OH, OW)
        for b, (x0, y0, f) in enumerate(wins):
            assert y0 + OH <= 34 or x0 + OW <= 46, 'the window must miss the corner'
            ref = full[b, :, y0:y0 + OH, x0:x0 + OW]
            ref = torch.flip(ref, dims=[-1]) if f else ref
            assert torch.equal(out[b], ref), f'window {wins[b]}'
            # (what a per-window normalisation would give differs)
            local = ops.isr_multi(gray[b:b + 1, y0:y0 + OH, x0:x0 + OW].contiguous(), VAL_RANGE, prm, 3).cpu()[0]
            local = torch.flip(local, dims=[-1]) if f else local
            assert not torch.equal(local, ref)


def test_isr_multi_refusals(tgt):
    from cmda_amd._lib import c_i32, ptr
    B, H, W = 2, 12, 16
    gray = tgt.to(_gray(B, H, W))
    lut = ops.isr_lut(VAL_RANGE, tgt.device)
    prm = ops.isr_multi_params(ROWS, 'rightdown', tgt.device, val_range=VAL_RANGE)
    mm = tgt.to(torch.zeros(B * 3 * 16, dtype=torch.int32))
    sentinel = 7.0
    out = tgt.to(torch.full((B, 3, H, W), sentinel))
    win = tgt.to(torch.tensor([[0, 0, 0], [2, 1, 1]], dtype=torch.int32))
    lib = _lib.lib()

    def run(C=3, nd=None, wc=None, win_=None, OH=H, OW=W, out_=out, gray_=gray, prm_=prm):
        ndc = (ctypes.c_int * len(nd))(*nd) if nd is not None else None
        wcc = (ctypes.c_int * len(wc))(*wc) if wc is not None else None
        return lib.cmdax4_isr_multi(ptr(gray_), ptr(lut), ptr(prm_), ptr(win_), ptr(mm), ptr(out_), ndc, wcc, c_i32(B), c_i32(C), c_i32(H),
                                    c_i32(W), c_i32(OH), c_i32(OW), _lib.stream_of(gray))
    SHAPE, UNSUP = -1, -4
    assert run(C=0) == SHAPE and run(C=4) == SHAPE, 'C outside 1..3'
    assert run(nd=[2, 3, 2]) == SHAPE and run(nd=[2, 2, 1]) == SHAPE and run(nd=[8, 2, 2]) == SHAPE, 'ndir outside {2, 4}'
    assert run(OH=H - 2) == SHAPE, 'a smaller output without a window'
    assert run(win_=win, OH=H + 1) == SHAPE and run(win_=win, OW=W + 1) == SHAPE
    assert run(win_=win, OH=8, OW=8, wc=[0, 0, 0, W - 7, 0, 0]) == SHAPE, 'a window that leaves the map on the right'
    assert run(win_=win, OH=8, OW=8, wc=[0, H - 7, 0, 0, 0, 0]) == SHAPE and run(win_=win, OH=8, OW=8, wc=[-1, 0, 0, 0, 0, 0]) == SHAPE
    assert run(win_=win, OH=8, OW=8, wc=[0, 0, 2, 0, 0, 0]) == SHAPE, 'flip is 0 or 1'
    assert run(out_=None) == UNSUP and run(gray_=None) == UNSUP and run(prm_=None) == UNSUP, 'null pointers'
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((B, 3, H, W), sentinel)), 'a refused call writes nothing'
    with pytest.raises(_lib.CmdaError):
        ops.isr_multi(gray, VAL_RANGE, prm, 3, window=win, out_size=(8, 8), window_host=[(0, 0, 0), (W - 7, 0, 0)])
    with pytest.raises(_lib.CmdaError):
        ops.isr_multi(gray, VAL_RANGE, prm, 3, ndir_host=[2, 2, 3])
    assert run(nd=[2, 2, 2]) == 0
    assert not (out.cpu() == sentinel).any()
    # a window only the device knows to be out of range is clamped into the map: nothing is read or written outside it
    bad = tgt.to(torch.tensor([[-5, 99, 0], [99, -5, 1]], dtype=torch.int32))
    got = ops.isr_multi(gray, VAL_RANGE, prm, 3, window=bad, out_size=(8, 8)).cpu()
    full = out.cpu()
    assert torch.equal(got[0], full[0, :, H - 8:, :8]) and torch.equal(got[1], torch.flip(full[1, :, :8, W - 8:], dims=[-1]))
