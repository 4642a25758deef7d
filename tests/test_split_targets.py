"""The split train type's target kernel pair (include/cmda_hip_ext6.h, ops.split_mix_targets): both streams' pseudo-labels, confident
counts, ClassMix'd labels and ClassMix'd weights in two launches.  The checker is the composed sequence of the existing ops
(ops.pseudo_label -> ops.pseudo_weight -> ops.class_mix_label / ops.class_mix) on the same target, per map: equality is exact."""
import ctypes

import pytest
import torch

from cmda_amd import _lib as L
from cmda_amd import ops

THR = 0.968
# (B, h, w, H, W): one partial 64 x 8 tile; a width and height that are no tile multiples; a tile seam; a non-integer factor
SHAPES = [(1, 4, 4, 16, 16), (2, 5, 19, 20, 76), (3, 8, 33, 16, 66), (1, 6, 10, 15, 27)]
K = 10
# logit scales per class count (image map, events map): chosen so that the confident share of either map is well inside (0, 1) at the
# threshold -- with 2 classes a pixel is confident from a score gap of log(0.968 / 0.032) = 3.4 on, with 19 from about 6.3 on
SCALES = {2: (3.0, 6.0), 19: (8.0, 16.0)}


def _inputs(B, h, w, H, W, nc, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * h + 7 * w + nc)
    s0, s1 = SCALES[nc]
    lg0 = torch.randn(B, h, w, nc, generator=g) * s0
    lg1 = torch.randn(B, h, w, nc, generator=g) * s1
    # source labels: blocks of one class (so that drawn classes cover regions), 255 among them
    pool = torch.tensor([0, 1, 2, 3, 5, 7, 11, 18, 255])
    coarse = pool[torch.randint(0, len(pool), (B, (H + 3) // 4, (W + 3) // 4), generator=g)]
    coarse[:, 0, 0], coarse[:, 0, 1] = 255, 2   # every sample has ignored pixels (drawn) and pixels of a class that is not drawn
    lab = coarse.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    classes = torch.full((B, K), -1, dtype=torch.int64)
    for b in range(B):
        pick = [255, 1, 5, 18] if b % 2 == 0 else [0, 255, 7]
        classes[b, :len(pick)] = torch.tensor(pick)
    return lg0, lg1, lab, classes


def _composed(tgt, lg, lab, classes, top, bottom):
    """the existing ops on one map: what uda.DACS._mix_targets runs"""
    B, H, W = lab.shape
    pseudo, _, count = ops.pseudo_label(lg, H, W, THR, want_prob=False)
    pw = ops.pseudo_weight(count, B, H, W, top, bottom)
    ones = torch.ones(B, H, W, dtype=torch.float32, device=lab.device)
    mixed = ops.class_mix_label(lab, pseudo, lab, classes)
    weight = ops.class_mix(ones.view(B, 1, H, W), pw.view(B, 1, H, W), lab, classes).view(B, H, W)
    return pseudo, count, mixed, weight


@pytest.mark.parametrize('tb', ['none', 'rows', 'all'])
@pytest.mark.parametrize('nc', [2, 19])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_split_targets_equal_composed_ops(tgt, shape, nc, tb):
    B, h, w, H, W = shape
    top, bottom = {'none': (0, 0), 'rows': (3, 2), 'all': (H, 0)}[tb]
    lg0, lg1, lab, classes = [tgt.to(t) for t in _inputs(*shape, nc)]
    ref = [_composed(tgt, lg, lab, classes, top, bottom) for lg in (lg0, lg1)]
    total = B * H * W
    c0, c1 = int(ref[0][1].item()), int(ref[1][1].item())
    assert 0 < c0 < total and 0 < c1 < total and c0 != c1, f'confident counts {c0}, {c1} of {total} do not tell the streams apart'
    in_drawn = (lab.cpu().view(B, 1, H, W) == classes.cpu().view(B, K, 1, 1)).any(1)
    assert 0 < int(in_drawn.sum()) < total and bool((lab.cpu()[in_drawn] == 255).any()), 'the draw covers part of the image, 255 included'
    pseudo, count, mixed, weight = ops.split_mix_targets(lg0, lg1, lab, classes, THR, top, bottom)
    assert pseudo.shape == mixed.shape == weight.shape == (2, B, H, W) and count.shape == (2,)
    assert pseudo.dtype == mixed.dtype == torch.int64 and count.dtype == torch.int32 and weight.dtype == torch.float32
    for s, name in enumerate(('image', 'events')):
        rp, rc, rm, rw = ref[s]
        assert torch.equal(pseudo[s].cpu(), rp.cpu()), f'{name} pseudo-label'
        assert int(count[s].item()) == int(rc.item()), f'{name} confident count'
        assert torch.equal(mixed[s].cpu(), rm.cpu()), f'{name} mixed label'
        assert torch.equal(weight[s].cpu(), rw.cpu()), f'{name} mixed weight'
    if tb == 'all':   # top + bottom covering every row: only the drawn classes keep a weight
        assert torch.equal(weight[0].cpu(), in_drawn.float()) and torch.equal(weight[1].cpu(), in_drawn.float())


def test_split_targets_identical_maps_give_identical_halves(tgt):
    lg0, _, lab, classes = [tgt.to(t) for t in _inputs(2, 5, 19, 20, 76, 19)]
    pseudo, count, mixed, weight = ops.split_mix_targets(lg0, lg0.clone(), lab, classes, THR, 3, 2)
    assert torch.equal(pseudo[0].cpu(), pseudo[1].cpu()) and torch.equal(mixed[0].cpu(), mixed[1].cpu())
    assert int(count[0].item()) == int(count[1].item()) and torch.equal(weight[0].cpu(), weight[1].cpu())


def test_split_targets_swapped_maps_swap_the_halves(tgt):
    lg0, lg1, lab, classes = [tgt.to(t) for t in _inputs(3, 8, 33, 16, 66, 19)]
    a = ops.split_mix_targets(lg0, lg1, lab, classes, THR, 3, 2)
    b = ops.split_mix_targets(lg1, lg0, lab, classes, THR, 3, 2)
    assert int(a[1][0].item()) != int(a[1][1].item()) and not torch.equal(a[0][0].cpu(), a[0][1].cpu())
    for x, y in zip(a, b):
        assert torch.equal(x.cpu(), y.flip(0).cpu())


def _raw(name, *args):
    return getattr(L.lib(), name)(*args)


def test_sixth_table_refusals(tgt):
    """every refusal is decided on the host before the launch: nothing is written"""
    i32, f32 = ctypes.c_int32, ctypes.c_float
    SHAPE, UNSUPPORTED = -1, -4
    B, h, w, H, W, nc = 1, 2, 2, 8, 8, 3
    lg = tgt.to(torch.randn(B, h, w, nc))
    lab = tgt.to(torch.zeros(B, H, W, dtype=torch.int64))
    classes = tgt.to(torch.full((B, K), -1, dtype=torch.int64))
    pseudo = tgt.to(torch.full((2, B, H, W), 7, dtype=torch.int64))
    mixed = tgt.to(torch.full((2, B, H, W), 7, dtype=torch.int64))
    weight = tgt.to(torch.full((2, B, H, W), 7.0))
    count = tgt.to(torch.full((2,), 7, dtype=torch.int32))
    p = L.ptr

    def targets(l0=lg, l1=lg, lb=lab, cl=classes, ps=pseudo, mx=mixed, ct=count, B=B, h=h, w=w, H=H, W=W, nc=nc, K=K):
        return _raw('cmdax6_split_targets', p(l0), p(l1), p(lb), p(cl), p(ps), p(mx), p(ct), i32(B), i32(h), i32(w), i32(H), i32(W),
                    i32(nc), i32(K), f32(THR), None)

    def weights(ct=count, lb=lab, cl=classes, wt=weight, B=B, H=H, W=W, K=K, top=0, bottom=0):
        return _raw('cmdax6_split_weights', p(ct), p(lb), p(cl), p(wt), i32(B), i32(H), i32(W), i32(K), i32(top), i32(bottom), None)

    for kw in (dict(nc=0), dict(nc=33), dict(nc=-1), dict(K=0), dict(K=-2), dict(B=0), dict(h=0), dict(w=0), dict(H=0), dict(W=-1),
               dict(B=2, H=1 << 15, W=1 << 15), dict(B=1 << 11, H=1 << 10, W=1 << 10)):
        assert targets(**kw) == SHAPE, kw
    for kw in (dict(l0=None), dict(l1=None), dict(lb=None), dict(cl=None), dict(ps=None), dict(mx=None), dict(ct=None)):
        assert targets(**kw) == UNSUPPORTED, kw
    for kw in (dict(K=0), dict(B=0), dict(H=0), dict(W=0), dict(top=-1), dict(bottom=-1), dict(B=2, H=1 << 15, W=1 << 15)):
        assert weights(**kw) == SHAPE, kw
    for kw in (dict(ct=None), dict(lb=None), dict(cl=None), dict(wt=None)):
        assert weights(**kw) == UNSUPPORTED, kw
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    for t in (pseudo, mixed, count):
        assert bool((t.cpu() == 7).all()), 'a refused call wrote'
    assert bool((weight.cpu() == 7.0).all()), 'a refused call wrote'
    # legal: 32 classes are the most; top + bottom beyond H zeroes everything outside the drawn classes (none drawn here)
    lg32 = tgt.to(torch.randn(B, h, w, 32))
    count.zero_()
    assert targets(l0=lg32, l1=lg32, nc=32) == 0
    assert weights(top=H, bottom=H) == 0
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert bool((weight.cpu() == 0).all())
    # the Python op refuses what the table cannot describe
    with pytest.raises(L.CmdaError):
        ops.split_mix_targets(lg, tgt.to(torch.randn(B, h, w, nc + 1)), lab, classes, THR)
    with pytest.raises(L.CmdaError):
        ops.split_mix_targets(lg, lg, lab.int(), classes, THR)
    with pytest.raises(L.CmdaError):
        ops.split_mix_targets(lg, lg, lab, classes[:, :0].contiguous(), THR)
