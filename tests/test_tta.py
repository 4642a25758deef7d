"""Sliding-window and multi-view (multi-scale / flip) evaluation on the device: `ops.seg_predict_windows`, `ops.seg_prob_accumulate`,
`ops.prob_predict` (include/cmda_hip_ext2.h), the segmentors' slide mode, `aug_test` / `predict_aug` and
`distributed_evaluate(on_device=True)` with `augs`.  The checker is plain torch on CPU (fp32, near-ties decided in float64), the
composition of the shipped ops (`slide_inference`, `simple_test`, `aug_test`) and the reference's own label maps
(tests/golden/tta.npz)."""
import functools
import hashlib
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import DACS_CH, DACS_DIMS, DACS_SEG_SCALE, seeded_fill, seeded_randn  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import _lib, metrics, ops, segmentors, uda  # noqa: E402
from cmda_amd._lib import CmdaError, c_i32, ptr  # noqa: E402
from cmda_amd.registry import build_segmentor  # noqa: E402
from conftest import check_le  # noqa: E402
import test_seg_eval as tse  # noqa: E402

SEED = 2025
NAMES = tse.NAMES

# ---------------------------------------------------------------------------------------------------------------------------
# kernels.  (B, nc, (H, W), crop, stride, (OH, OW), low-resolution window size or None = ceil(window / 4))
CASES = {
    'clamped': (2, 19, (44, 72), (32, 48), (20, 32), (44, 72), None),    # 4 windows, last row / column shifted back, counts {1,2,4}
    'dense': (1, 19, (56, 48), (32, 32), (8, 16), (60, 50), None),       # 8 windows, counts {1,2,3,4,6,8}, non-integer second stage
    'big_crop': (1, 19, (44, 72), (64, 96), (40, 60), (44, 72), None),   # crop larger than the image: one window
    'nc32': (1, 32, (40, 40), (24, 24), (16, 16), (37, 45), None),       # nc at the limit
    'nc1': (1, 1, (40, 40), (24, 24), (16, 16), (37, 45), None),         # a single class
    'down': (1, 5, (10, 40), (8, 24), (2, 16), (10, 40), (32, 96)),      # down-sampling windows: rows beyond the LDS budget
}
FLIPS = (0, 1, 2)
CASE_FLIPS = [(name, flip) for name in CASES for flip in FLIPS]


def _sync(tgt):
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()


def _win_hw(name):
    _, _, (H, W), crop, _, _, low = CASES[name]
    ch, cw = min(crop[0], H), min(crop[1], W)
    return (ch, cw), (low if low is not None else (math.ceil(ch / 4), math.ceil(cw / 4)))


@functools.lru_cache(maxsize=None)
def _logits(name):
    B, nc, hw, crop, stride, _, _ = CASES[name]
    K = len(ops.slide_windows(hw[0], hw[1], crop, stride))
    (hl, wl) = _win_hw(name)[1]
    return torch.randn((K, B, hl, wl, nc), generator=torch.Generator().manual_seed(SEED + sorted(CASES).index(name))) * 4


def _flip(t, flip):
    return t if flip == 0 else t.flip(dims=(-1,) if flip == 1 else (-2,))


def _slide_scores(lg, hw, crop, stride, out_hw, upsample):
    """the reference's slide_inference (encoder_decoder.py:175-218): preds = 0; preds += pad(up-sampled window logits) in window
    order; preds /= count; resize to out_hw.  `upsample(nhwc, h, w)` -> NCHW and `resize(nchw, hw)` are the caller's."""
    up, resize = upsample
    K, B, _, _, nc = lg.shape
    H, W = hw
    wins = ops.slide_windows(H, W, crop, stride)
    assert len(wins) == K
    preds = count = None
    for k, (y1, x1, y2, x2) in enumerate(wins):
        u = up(lg[k], y2 - y1, x2 - x1)
        if preds is None:
            preds, count = u.new_zeros(B, nc, H, W), u.new_zeros(B, 1, H, W)
        preds += F.pad(u, (x1, W - x2, y1, H - y2))
        count[:, :, y1:y2, x1:x2] += 1
    assert int((count == 0).sum()) == 0
    preds = preds / count
    return resize(preds, out_hw) if tuple(out_hw) != (H, W) else preds


def _torch_ops(dtype):
    up = lambda t, h, w: F.interpolate(t.permute(0, 3, 1, 2).to(dtype), size=(h, w), mode='bilinear', align_corners=False)
    return up, lambda s, hw: F.interpolate(s, size=hw, mode='bilinear', align_corners=False)


_SHIPPED_OPS = (lambda t, h, w: ops.upsample_logits_nchw(t.contiguous(), h, w), lambda s, hw: segmentors._resize_logits(s, hw))


@functools.lru_cache(maxsize=None)
def _torch_reference(name):
    """(fp32 labels before the flip-back, near-tie mask from float64) -- computed once per case"""
    _, _, hw, crop, stride, out_hw, _ = CASES[name]
    lg = _logits(name)
    s32 = _slide_scores(lg, hw, crop, stride, out_hw, _torch_ops(torch.float32))
    lab = torch.softmax(s32, dim=1).argmax(dim=1)
    assert torch.equal(lab, s32.argmax(dim=1))          # the soft-max is monotone: skipping it changes no label of the reference
    s64 = _slide_scores(lg, hw, crop, stride, out_hw, _torch_ops(torch.float64))
    if lg.shape[-1] == 1:
        return lab, torch.zeros_like(lab, dtype=torch.bool)
    top2 = s64.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < 1e-5 * lg.abs().max().double()
    assert torch.equal(lab[~near], s64.argmax(dim=1)[~near])
    return lab, near


def _windows(tgt, name, flip=0, **kw):
    _, _, hw, crop, stride, out_hw, _ = CASES[name]
    return ops.seg_predict_windows(tgt.to(_logits(name)), hw[0], hw[1], crop, stride, out_hw, flip, **kw)


def test_slide_windows_grid():
    """the grids the cases are meant to cover"""
    for name, k, counts in (('clamped', 4, {1, 2, 4}), ('dense', 8, {1, 2, 3, 4, 6, 8}), ('big_crop', 1, {1}), ('nc32', 4, {1, 2, 4})):
        _, _, (H, W), crop, stride, _, _ = CASES[name]
        wins = ops.slide_windows(H, W, crop, stride)
        count = torch.zeros(H, W, dtype=torch.long)
        for y1, x1, y2, x2 in wins:
            assert 0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W and (y2 - y1, x2 - x1) == (min(crop[0], H), min(crop[1], W))
            count[y1:y2, x1:x2] += 1
        assert len(wins) == k and set(count.unique().tolist()) == counts, (name, len(wins), count.unique())
    assert ops.slide_windows(44, 72, (32, 48), (20, 32)) == [(0, 0, 32, 48), (0, 24, 32, 72), (12, 0, 44, 48), (12, 24, 44, 72)]


@pytest.mark.parametrize('name,flip', CASE_FLIPS)
def test_windows_match_torch(tgt, name, flip):
    """labels of the fused kernel = torch's restatement of slide_inference (interpolate per window, pad, add, divide, interpolate)
    + softmax + flip + argmax at every pixel whose float64 top-2 gap is at least 1e-5 * max|logits|; at most 1e-3 of the pixels may
    be that close"""
    lab, near = _torch_reference(name)
    got = _windows(tgt, name, flip)
    _sync(tgt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(lab.shape)
    check_le(f'{name}: near-tie share', near.double().mean().item(), 1e-3)
    want, skip = _flip(lab, flip), _flip(near, flip)
    bad = (got.cpu().long() != want) & ~skip
    assert int(bad.sum()) == 0, f'{name} flip {flip}: {int(bad.sum())} labels differ outside near-ties'


def _shipped_scores(tgt, name):
    """S2 of the composition of the shipped ops (what `slide_inference` computes), on the target"""
    _, _, hw, crop, stride, out_hw, _ = CASES[name]
    return _slide_scores(tgt.to(_logits(name)), hw, crop, stride, out_hw, _SHIPPED_OPS)


def _tie(values):
    """pixels whose two largest values over dim 1 are bitwise equal"""
    if values.shape[1] == 1:
        return torch.zeros(values.shape[:1] + values.shape[2:], dtype=torch.bool)
    top2 = values.topk(2, dim=1).values
    return (top2[:, 0] == top2[:, 1]).cpu()


@pytest.mark.parametrize('name', list(CASES))
def test_windows_equal_existing_path(tgt, name):
    """the same arithmetic as the composition of the shipped ops: upsample_logits_nchw per window, torch add and divide,
    _resize_logits, softmax, flip, argmax -- equal wherever that path's two largest values are not bitwise equal"""
    old = _shipped_scores(tgt, name)
    for flip in FLIPS:
        prob = torch.softmax(_flip(old, flip), dim=1)
        tie = _tie(prob)
        got = _windows(tgt, name, flip)
        _sync(tgt)
        check_le(f'{name} flip {flip}: tied share of the old path', tie.double().mean().item(), 1e-3)
        assert torch.equal(got.cpu().long()[~tie], prob.argmax(dim=1).cpu()[~tie])


@pytest.mark.parametrize('name', ['one_stage', 'two_stage'])
def test_single_window_equals_seg_predict(tgt, name):
    """a crop that covers the image: the labels and counters of the shipped whole-image kernel, bit for bit"""
    _, hw, out_hw, flips = tse.CASES[name]
    lg = tgt.to(tse._logits(name))
    nc = lg.shape[-1]
    gt = tgt.to(torch.randint(0, nc, (lg.shape[0],) + tuple(out_hw), generator=torch.Generator().manual_seed(SEED)))
    for flip in flips:
        for crop, stride in ((hw, hw), ((hw[0] + 20, hw[1] + 3), (7, 1000))):
            a, b = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device), torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
            got = ops.seg_predict_windows(lg[None], hw[0], hw[1], crop, stride, out_hw, flip, gt, a)
            want = ops.seg_predict(lg, hw[0], hw[1], out_hw, flip, gt, b)
            _sync(tgt)
            assert torch.equal(got, want) and torch.equal(a, b), (name, flip, crop)


def _softmax_bound(scores):
    """fp64 soft-max of fp32 scores and the bound of the probability checks: 4 x the error torch's own fp32 soft-max shows on
    these scores (the margin for a different exp) + 2^-23"""
    scores = scores.cpu()
    p64 = torch.softmax(scores.double(), dim=1)
    own = (torch.softmax(scores, dim=1).double() - p64).abs().max().item()
    return p64, 4 * own + 2.0 ** -23


@pytest.mark.parametrize('name', list(CASES))
def test_prob_accumulate(tgt, name):
    """acc after one write (a pre-filled acc is overwritten), and after the write plus two accumulates with the other flips"""
    B, nc, hw, crop, stride, out_hw, _ = CASES[name]
    lg = tgt.to(_logits(name))
    p64, bound = _softmax_bound(_shipped_scores(tgt, name))
    acc = torch.full((B, nc) + tuple(out_hw), 7.0, device=tgt.device)
    assert ops.seg_prob_accumulate(lg, hw[0], hw[1], crop, stride, out_hw, 1, acc, False) is acc
    _sync(tgt)
    check_le(f'{name}: probabilities of one view', (acc.cpu().double() - _flip(p64, 1)).abs().max().item(), bound)
    ops.seg_prob_accumulate(lg, hw[0], hw[1], crop, stride, out_hw, 0, acc, True)
    ops.seg_prob_accumulate(lg, hw[0], hw[1], crop, stride, out_hw, 2, acc, True)
    _sync(tgt)
    want = _flip(p64, 1) + p64 + _flip(p64, 2)
    # (three terms of at most 1 and two fp32 additions of sums below 4: 2 x 2^-23 on top)
    check_le(f'{name}: probabilities summed over three views', (acc.cpu().double() - want).abs().max().item(), 3 * bound + 2 * 2.0 ** -23)


@functools.lru_cache(maxsize=None)
def _acc_and_gt(nc=19, shape=(2, 37, 70)):
    gen = torch.Generator().manual_seed(SEED + 5)
    acc = torch.softmax(torch.randn(shape[0], nc, shape[1], shape[2], generator=gen) * 2, dim=1)
    acc = acc + torch.softmax(torch.randn(acc.shape, generator=gen) * 2, dim=1) + torch.softmax(torch.randn(acc.shape, generator=gen), dim=1)
    acc[0, 3, :4] = acc[0, 5, :4] = 3.5                 # exact ties: the first arg-max wins
    gt = torch.randint(0, nc, shape, generator=gen)
    gt[torch.rand(shape, generator=gen) < 0.1] = 255
    return acc, gt


@pytest.mark.parametrize('n', [1, 3])
def test_prob_predict(tgt, n):
    """labels = argmax(acc / n) outside bitwise ties of acc / n; at the planted ties the first class; fused counters = the
    counters of the returned labels"""
    acc, gt = _acc_and_gt()
    nc = acc.shape[1]
    dacc = tgt.to(acc)
    mean = dacc / n
    tie = _tie(mean)
    got = ops.prob_predict(dacc, n)
    _sync(tgt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 37, 70)
    assert torch.equal(got.cpu().long()[~tie], mean.argmax(dim=1).cpu()[~tie])
    assert bool((got[0, :4] == 3).all()) and bool(tie[0, :4].all())
    two = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
    ops.confusion_update(got, tgt.to(gt), two, nc, 255)
    for dt in (torch.uint8, torch.int64):
        conf = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
        out = torch.empty_like(got)
        assert ops.prob_predict(dacc, n, tgt.to(gt.to(dt)), conf, 255, out=out) is out
        _sync(tgt)
        assert torch.equal(out, got) and torch.equal(conf, two) and int(conf.sum()) == int((gt != 255).sum()), dt
        ops.prob_predict(dacc, n, tgt.to(gt.to(dt)), conf, 255)         # a second call accumulates
        assert torch.equal(conf, 2 * two), dt


@pytest.mark.parametrize('name', ['clamped', 'dense'])
def test_windows_fused_score_equals_two_step(tgt, name):
    """seg_predict_windows with gt / conf = seg_predict_windows, then confusion_update"""
    B, nc, _, _, _, out_hw, _ = CASES[name]
    gen = torch.Generator().manual_seed(SEED + 7)
    gt = torch.randint(0, nc, (B,) + tuple(out_hw), generator=gen)
    gt[torch.rand(gt.shape, generator=gen) < 0.1] = 255
    gt[torch.rand(gt.shape, generator=gen) < 0.05] = 200
    for flip in (0, 1):
        plain = _windows(tgt, name, flip)
        two = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
        ops.confusion_update(plain, tgt.to(gt), two, nc, 255)
        for dt in (torch.uint8, torch.int64):
            conf = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
            fused = _windows(tgt, name, flip, gt=tgt.to(gt.to(dt)), conf=conf, ignore_index=255)
            _sync(tgt)
            assert torch.equal(fused, plain) and torch.equal(conf, two), (flip, dt)
            assert int(conf.sum()) == int((gt != 255).sum())
            _windows(tgt, name, flip, gt=tgt.to(gt.to(dt)), conf=conf, ignore_index=255)
            assert torch.equal(conf, 2 * two), (flip, dt)


def test_tta_refusals(tgt):
    """every refusal is an error code without a launch: CmdaError, label_out, acc and conf untouched"""
    nc = 19
    lg = tgt.to(torch.randn(4, 1, 2, 2, nc))            # 8 x 8 image, crop 6, stride 2: 2 x 2 windows
    out = tgt.to(torch.full((1, 8, 8), 7, dtype=torch.uint8))
    acc = tgt.to(torch.full((1, nc, 8, 8), 5.0))
    conf = tgt.to(torch.full((nc + 1, nc), 3, dtype=torch.int64))
    gt = tgt.to(torch.zeros(1, 8, 8, dtype=torch.uint8))

    def raw_scores(mode=0, out_=out, acc_=None, B=1, hl=2, wl=2, H=8, W=8, ch=6, cw=6, sh=2, sw=2, OH=8, OW=8, nc_=nc, flip=0,
                   gt_=None, tag=0, conf_=None):
        _lib.call('cmdax2_seg_scores', ptr(lg), c_i32(mode), ptr(out_), ptr(acc_), c_i32(0), ptr(gt_), c_i32(tag), ptr(conf_), c_i32(B),
                  c_i32(hl), c_i32(wl), c_i32(H), c_i32(W), c_i32(ch), c_i32(cw), c_i32(sh), c_i32(sw), c_i32(OH), c_i32(OW), c_i32(nc_),
                  c_i32(flip), c_i32(255), _lib.stream_of(lg))

    def raw_predict(B=1, OH=8, OW=8, nc_=nc, n=2, gt_=None, tag=0, conf_=None):
        _lib.call('cmdax2_prob_predict', ptr(acc), ptr(out), ptr(gt_), c_i32(tag), ptr(conf_), c_i32(B), c_i32(OH), c_i32(OW),
                  c_i32(nc_), c_i32(n), c_i32(255), _lib.stream_of(lg))
    big = 1 << 20
    refused = [
        lambda: raw_scores(nc_=33), lambda: raw_scores(nc_=0), lambda: raw_scores(B=-1),
        lambda: raw_scores(OH=46341, OW=46341),                        # B * OH * OW >= 2^31
        lambda: raw_scores(B=2, OH=32768, OW=32768),
        lambda: raw_scores(H=big, W=big, ch=1, cw=1, sh=16, sw=16),     # K >= 2^31
        lambda: raw_scores(B=4, H=big, W=big, ch=1, cw=1, sh=64, sw=32),   # K * B >= 2^31
        lambda: raw_scores(hl=0), lambda: raw_scores(wl=0), lambda: raw_scores(H=0), lambda: raw_scores(W=-1),
        lambda: raw_scores(OH=0), lambda: raw_scores(OW=0),
        lambda: raw_scores(ch=0), lambda: raw_scores(cw=-3), lambda: raw_scores(sh=0), lambda: raw_scores(sw=0),
        lambda: raw_scores(flip=3), lambda: raw_scores(flip=-1), lambda: raw_scores(mode=2), lambda: raw_scores(mode=-1),
        lambda: raw_scores(gt_=gt, tag=2, conf_=conf),                 # bad dtype tag
        lambda: raw_scores(conf_=conf), lambda: raw_scores(gt_=gt),    # one of gt / conf without the other
        lambda: raw_scores(mode=1, acc_=acc, gt_=gt, conf_=conf),      # a confusion update in probability mode
        lambda: raw_scores(mode=1, acc_=acc, conf_=conf), lambda: raw_scores(mode=1, acc_=acc, gt_=gt),
        lambda: raw_scores(mode=1, acc_=None), lambda: raw_scores(mode=0, out_=None, acc_=acc),   # the mode's output missing
        lambda: raw_predict(nc_=33), lambda: raw_predict(nc_=0), lambda: raw_predict(n=0), lambda: raw_predict(n=-2),
        lambda: raw_predict(B=-1), lambda: raw_predict(OH=0), lambda: raw_predict(OW=0), lambda: raw_predict(OH=46341, OW=46341),
        lambda: raw_predict(gt_=gt, tag=2, conf_=conf), lambda: raw_predict(conf_=conf), lambda: raw_predict(gt_=gt),
        # the same through the public functions
        lambda: ops.seg_predict_windows(tgt.to(torch.randn(4, 1, 2, 2, 33)), 8, 8, (6, 6), (2, 2), out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (2, 2), flip=3, out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (2, 2), conf=conf, out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (2, 2), gt=gt, out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (2, 2), gt=gt.int(), conf=conf, out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (0, 2), out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (0, 6), (2, 2), out=out),
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (1, 2), out=out),                 # 3 x 2 windows, 4 given
        lambda: ops.seg_predict_windows(lg[0], 8, 8, (6, 6), (2, 2), out=out),               # not [K,B,hl,wl,nc]
        lambda: ops.seg_predict_windows(lg, 8, 8, (6, 6), (2, 2), out=out[:, :4]),
        lambda: ops.seg_prob_accumulate(lg, 8, 8, (6, 6), (2, 2), (8, 8), 5, acc, False),
        lambda: ops.seg_prob_accumulate(lg, 8, 8, (6, 6), (2, 2), (8, 9), 0, acc, False),
        lambda: ops.seg_prob_accumulate(lg, 8, 8, (6, 6), (2, 2), (8, 8), 0, acc.double(), False),
        lambda: ops.slide_windows(8, 8, (6, 6), (0, 2)),
        lambda: ops.prob_predict(acc, 0, out=out), lambda: ops.prob_predict(acc, 2, gt=gt, out=out),
        lambda: ops.prob_predict(acc, 2, conf=conf, out=out), lambda: ops.prob_predict(acc, 2, gt=gt.float(), conf=conf, out=out),
        lambda: ops.prob_predict(acc[0], 2, out=out), lambda: ops.prob_predict(tgt.to(torch.ones(1, 33, 8, 8)), 2, out=out),
    ]
    for i, f in enumerate(refused):
        with pytest.raises(CmdaError):
            f()
            pytest.fail(f'refusal {i} went through')
    _sync(tgt)
    assert bool((out == 7).all()) and bool((conf == 3).all()) and bool((acc == 5).all())
    raw_scores(gt_=gt, conf_=conf)                       # (the same arguments, valid: they run)
    _sync(tgt)
    assert int(out.max()) < nc and int(conf.sum()) == 3 * conf.numel() + 64
    raw_scores(mode=1, acc_=acc)
    _sync(tgt)
    assert float((acc.sum(dim=1) - 1).abs().max()) < 1e-5
    out.fill_(7)
    raw_predict(gt_=gt, conf_=conf)
    _sync(tgt)
    assert int(out.max()) < nc and int(conf.sum()) == 3 * conf.numel() + 128
    # the product binding has no CPU fallback
    _lib._unbind_for_tests()
    with pytest.raises(CmdaError, match='no CPU fallback'):
        ops.seg_predict_windows(torch.randn(4, 1, 2, 2, nc), 8, 8, (6, 6), (2, 2))
    with pytest.raises(CmdaError, match='no CPU fallback'):
        ops.seg_prob_accumulate(torch.randn(4, 1, 2, 2, nc), 8, 8, (6, 6), (2, 2), (8, 8), 0, torch.zeros(1, nc, 8, 8), False)
    with pytest.raises(CmdaError, match='no CPU fallback'):
        ops.prob_predict(torch.ones(1, nc, 8, 8), 2)


# ---------------------------------------------------------------------------------------------------------------------------
# segmentors: the SMALL model, the input size and the metas of test_seg_eval.py
KINDS = ['fusion', 'events', 'plain']
SLIDE = dict(mode='slide', crop_size=(48, 64), stride=(16, 32))    # 2 x 2 windows on 64 x 96, both last windows shifted back
IN_HW, METAS = tse.IN_HW, tse.METAS


def _memoize_network(model):
    """the network's forward pass (deterministic, and not what these tests are about) runs once per distinct input batch: every path
    under test -- simple_test, inference, aug_test, predict, predict_aug -- still crops and batches the windows itself, asks the
    model for their logits and applies its own tail.  (test_seg_eval.py's memo keys on the identity of the input tensors; a batch
    of windows is a new tensor every time, so this one keys on the bytes.)"""
    def digest(a):
        if not isinstance(a, torch.Tensor):
            return repr(a)
        return (tuple(a.shape), str(a.dtype), hashlib.sha1(a.detach().cpu().contiguous().numpy().tobytes()).hexdigest())

    def wrap(name):
        fn, memo = getattr(model, name), {}

        def cached(*args, **kw):
            key = tuple(digest(a) for a in args) + tuple((k, digest(v)) for k, v in sorted(kw.items()))
            if key not in memo:
                memo[key] = fn(*args, **kw)
            return memo[key]
        setattr(model, name, cached)
    wrap('encode_decode_lowres')
    if type(model).__name__ == 'EncoderDecoder':
        wrap('encode_decode')
    return model


def _build(kind, tgt, test_cfg):
    model = tse._build(kind, tgt)
    model.test_cfg = dict(test_cfg)
    return _memoize_network(model)


def _host_labels(kind, model, kw, rescale=True):
    return torch.from_numpy(np.stack(model.simple_test(rescale, **kw) if kind != 'plain' else
                                     model.simple_test(kw['img'], kw['img_meta'], rescale)))


def _host_probs(kind, model, kw):
    return model.inference(True, **kw) if kind != 'plain' else model.inference(kw['img'], kw['img_meta'], True)


def _check_meter(meter, want, gt, tie):
    """the meter's metrics = metrics.mean_iou of the host labels (the slack rule of test_seg_eval.py)"""
    res, ref = meter.compute(), metrics.mean_iou([w for w in want], [gt], 19, 255)
    slack = float(tie.sum()) / float((gt != 255).sum())
    for k in NAMES:
        a, b = res[k].cpu().numpy(), ref[k].numpy()
        if slack == 0:
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        elif k == 'aAcc':   # (a pixel moves the overall accuracy by at most 1 / labelled pixels)
            assert abs(float(a) - float(b)) <= slack + 1e-12


def _gt(gen, oh, ow):
    gt = torch.randint(0, 19, (oh, ow), generator=gen)
    gt[torch.rand(oh, ow, generator=gen) < 0.1] = 255
    return gt


@pytest.mark.parametrize('kind', KINDS)
def test_slide_predict_matches_simple_test(tgt, kind):
    """test_cfg.mode 'slide': `predict` (the windows as one batch + one fused launch) = `simple_test` (slide_inference: full-size
    logits per window, pad, add, divide, resize) outside the bitwise ties of `inference`'s output; the meter = the host metric"""
    assert len(ops.slide_windows(IN_HW[0], IN_HW[1], SLIDE['crop_size'], SLIDE['stride'])) == 4
    rt.set_compute_dtype(torch.float32)
    model = _build(kind, tgt, SLIDE)
    gen = torch.Generator().manual_seed(SEED + 11)
    for meta in METAS:
        kw = tse._inputs(kind, tgt, meta)
        oh, ow = meta['ori_shape'][:2]
        gt = _gt(gen, oh, ow)
        with torch.no_grad():
            want = _host_labels(kind, model, kw)
            tie = _tie(_host_probs(kind, model, kw))
        meter = metrics.ConfusionMeter(19, 255, device=tgt.device)
        got = model.predict(True, gt_semantic_seg=gt, meter=meter, **kw)
        assert got.dtype == torch.uint8 and got.device.type == tgt.device.type and tuple(got.shape) == (1, oh, ow) == tuple(want.shape)
        check_le(f'{kind} {meta}: tied share of simple_test', tie.double().mean().item(), 1e-3)
        assert torch.equal(got.cpu().long()[~tie], want[~tie])
        _check_meter(meter, want, gt, tie)
    kw = tse._inputs(kind, tgt, METAS[1])
    full = model.predict(True, **kw)
    # rescale=False: labels at the input size, and the host path agrees
    small = model.predict(False, **kw)
    assert tuple(small.shape) == (1,) + IN_HW
    with torch.no_grad():
        assert tuple(_host_labels(kind, model, kw, False).shape) == (1,) + IN_HW
    # the reference's loop (one window per pass) against all windows as one batch: label maps of the same model through different
    # launch shapes -- the bound of test_seg_eval.py::test_predict_against_reference_gpu
    assert model.slide_batch is None
    model.slide_batch = 1
    looped = model.predict(True, **kw)
    model.slide_batch = None
    check_le(f'{kind}: slide_batch=1 against one batch, label disagreement', (looped != full).double().mean().item(), 1e-3)
    # a slide config without crop_size / stride is not a configuration
    for bad in (dict(mode='slide'), dict(mode='slide', crop_size=(48, 64)), dict(mode='slide', stride=(16, 32)), dict(mode='tile')):
        model.test_cfg = bad
        with pytest.raises(NotImplementedError):
            model.predict(True, **kw)
        with pytest.raises(NotImplementedError):
            _host_labels(kind, model, kw)


def _views(kind, tgt, seed=151):
    """three views of one image: scale 1.0, scale 1.0 flipped, a 48 x 72 input; all rescaled to the image's ori_shape"""
    img, ev = tse._input_tensors(tgt.kind) if seed == 151 else (
        tgt.to(seeded_randn((1, 3) + IN_HW, seed, 'img')), tgt.to(seeded_randn((1, 3) + IN_HW, seed, 'ev').clamp(-1, 1)))
    ori = (72, 100, 3)
    small = lambda t: F.interpolate(t, size=(48, 72), mode='bilinear', align_corners=False)
    out = []
    for f, meta in ((lambda t: t, dict(ori_shape=ori, flip=False)),
                    (lambda t: t.flip(dims=(3,)).contiguous(), dict(ori_shape=ori, flip=True, flip_direction='horizontal')),
                    (small, dict(ori_shape=ori, flip=False))):
        if kind == 'fusion':
            out.append(dict(warp_image=f(img), events_vg=f(ev), img_metas=meta))
        elif kind == 'events':
            out.append(dict(image=f(img), img_metas=meta))
        else:
            out.append(dict(img=f(img), img_meta=meta))
    return out


def _aug_host(kind, model, views):
    if kind == 'plain':
        return model.aug_test([v['img'] for v in views], [v['img_meta'] for v in views])
    return model.aug_test(views)


@pytest.mark.parametrize('mode', ['whole', 'slide'])
@pytest.mark.parametrize('kind', KINDS)
def test_predict_aug_matches_aug_test(tgt, kind, mode):
    """`predict_aug` (one launch per view + one) = `aug_test` (host label maps) outside the bitwise ties of the averaged
    probabilities"""
    rt.set_compute_dtype(torch.float32)
    model = _build(kind, tgt, SLIDE if mode == 'slide' else dict(mode='whole'))
    views = _views(kind, tgt)
    gt = _gt(torch.Generator().manual_seed(SEED + 17), 72, 100)
    with torch.no_grad():
        want = torch.from_numpy(np.stack(_aug_host(kind, model, views)))
        avg = _host_probs(kind, model, views[0])
        for v in views[1:]:
            avg += _host_probs(kind, model, v)
        avg /= len(views)
    assert torch.equal(want, avg.argmax(dim=1).cpu())
    tie = _tie(avg)
    meter = metrics.ConfusionMeter(19, 255, device=tgt.device)
    got = model.predict_aug(views, gt_semantic_seg=gt, meter=meter)
    assert got.dtype == torch.uint8 and got.device.type == tgt.device.type and tuple(got.shape) == (1, 72, 100) == tuple(want.shape)
    assert torch.equal(model.predict_aug(views), got)
    check_le(f'{kind} {mode}: tied share of aug_test', tie.double().mean().item(), 1e-3)
    assert torch.equal(got.cpu().long()[~tie], want[~tie])
    _check_meter(meter, want, gt, tie)
    # one view: the labels of predict
    assert torch.equal(model.predict_aug(views[1:2]), model.predict(True, **views[1]))
    # both multi-view calls insist on rescale, as the reference does
    with pytest.raises(AssertionError):
        model.aug_test([v['img'] for v in views], [v['img_meta'] for v in views], False) if kind == 'plain' else model.aug_test(views, False)
    # the UDA wrapper hands over to its student
    stub = types.SimpleNamespace(get_model=lambda: model)
    m2 = metrics.ConfusionMeter(19, 255, device=tgt.device)
    assert torch.equal(uda.DACS.predict_aug(stub, views, gt_semantic_seg=gt, meter=m2), got) and torch.equal(m2.conf, meter.conf)
    host2 = uda.DACS.aug_test(stub, [v['img'] for v in views], [v['img_meta'] for v in views]) if kind == 'plain' else uda.DACS.aug_test(stub, views)
    assert torch.equal(torch.from_numpy(np.stack(host2)), want)


@pytest.mark.parametrize('mode', ['whole', 'slide'])
def test_distributed_evaluate_augs_on_device(tgt, mode):
    """samples that carry `augs`: on_device=True (predict_aug) returns what the host path returns through a predict= hook that calls
    aug_test; a sample without `augs` still goes through predict"""
    from cmda_amd.parallel import distributed_evaluate
    rt.set_compute_dtype(torch.float32)
    model = _build('events', tgt, SLIDE if mode == 'slide' else dict(mode='whole')).train()
    gen = torch.Generator().manual_seed(SEED + 19)
    samples = [dict(augs=_views('events', tgt, 170 + i), gt_semantic_seg=_gt(gen, 72, 100)) for i in range(2)]
    samples.append(dict(tse._eval_samples(tgt)[1]))
    hook = lambda m, s: m.aug_test(s['augs'])[0] if 'augs' in s else m.simple_test(True, **s)[0]
    host = distributed_evaluate(model, samples, 19, 255, predict=hook)
    dev = distributed_evaluate(model, samples, 19, 255, on_device=True)
    assert model.training                                # the caller's state is restored
    tse._same(dev, host)


@pytest.mark.gpu
def test_slide_and_aug_against_reference_gpu():
    """tests/golden/tta.npz (make_golden_tta.py): the reference's own plain EncoderDecoder under test_cfg.mode 'slide' (crop 256,
    stride 192: 2 x 3 windows) at 440 x 640 -- simple_test with the flip off and on, aug_test over {440 x 640, flipped, 330 x 480}.
    Outside the fixture's mask (reference top-2 gap below 1e-3 of the top score) at most 1e-3 of the labels may differ: the bound
    of test_seg_eval.py::test_predict_against_reference_gpu."""
    from test_image_uda import SEEDS, _gpu, golden, model_cfg
    _gpu()
    ORI, IMG_SEED = (440, 640, 3), 142                   # (make_golden_tta.py's)
    g = golden('tta.npz')
    rt.set_compute_dtype(torch.float32)
    m = build_segmentor(dict(model_cfg(DACS_DIMS, DACS_CH), type='EncoderDecoder', test_cfg=dict(mode='slide', crop_size=(256, 256), stride=(192, 192))))
    seeded_fill(m, SEEDS['simple'])
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    m = m.cuda().eval()
    img = seeded_randn((1, 3, 440, 640), IMG_SEED, 'img').cuda()

    def check(name, seg):
        assert seg.dtype == torch.uint8 and seg.is_cuda and tuple(seg.shape) == (1, 440, 640)
        seg = seg.cpu().numpy()[..., ::4, ::4]   # (the fixture keeps every fourth row / column)
        ref, keep = g[name].numpy(), g['mask.' + name].numpy() == 0
        check_le(f'{name}: label disagreement outside the mask', ((seg != ref) & keep).sum() / keep.sum(), 1e-3)
    for flip in (False, True):
        check(f'slide.flip{int(flip)}', m.predict(True, img=img, img_meta=dict(ori_shape=ORI, flip=flip, flip_direction='horizontal')))
    plain, flipped = dict(ori_shape=ORI, flip=False), dict(ori_shape=ORI, flip=True, flip_direction='horizontal')
    small = F.interpolate(img, size=(330, 480), mode='bilinear', align_corners=False)
    check('aug', m.predict_aug([dict(img=img, img_meta=plain), dict(img=img.flip(dims=(3,)).contiguous(), img_meta=flipped),
                                dict(img=small, img_meta=plain)]))
