"""The fifth ABI table (cmda_amd/csrc/voxel_ordered.hip, include/cmda_hip_ext5.h): batched event preparation, the ORDER-PRESERVING
voxel grid and the batched events_norm, with the Python layers on top (ops, pipeline.events_voxel_batch, DSECDataset(ordered_events)).

"Bitwise" below is torch.equal against oracle.uda.events_to_voxel_grid on the CPU, no tolerance: the reference adds a cell's
contributions one at a time in fp32 (eight put_(accumulate=True) passes in corner order, each in event order), every operation of a
contribution is a single IEEE fp32 operation with contraction off, so there is exactly one right answer per cell and only a kernel
that keeps the order can give it (a permuted order changes ~94 % of the cells of the dense case, by up to 2e-5)."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest
import torch

import cmda_amd  # noqa: F401
from cmda_amd import _lib as L
from cmda_amd import datasets as D
from cmda_amd import ops, pipeline as pl
from conftest import assert_close
from oracle import uda as ouda

HERE = os.path.dirname(os.path.abspath(__file__))
HOT = (5.37, 3.61)


def oracle_grid(ev, W, H, bins):
    """oracle.uda.events_to_voxel_grid as the SEQUENTIAL sum it stands for.  torch's CPU put_(accumulate=True) adds one index at a
    time in index order -- except that from 32768 indices on, with more than one thread, it splits them over the threads; the
    deterministic-algorithms switch keeps it serial at every size (as it is in the reference's single-threaded loader workers)."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        return ouda.events_to_voxel_grid(*ev, W, H, bins)
    finally:
        torch.use_deterministic_algorithms(was)


def _times(g, N):
    """N sorted, distinct fp32 times in [0, 1)"""
    return torch.sort(torch.randperm(1 << 20, generator=g)[:N])[0].float() / float(1 << 20)


@functools.lru_cache(maxsize=None)
def dense_case(bins, N=20000, H=12, W=16):
    g = torch.Generator().manual_seed(bins)
    ev = (_times(g, N), torch.rand(N, generator=g) * (W - 1), torch.rand(N, generator=g) * (H - 1),
          torch.randint(0, 2, (N,), generator=g).float())
    return ev, oracle_grid(ev, W, H, bins)


@functools.lru_cache(maxsize=None)
def hot_case(N, bins, H=12, W=16):
    g = torch.Generator().manual_seed(N)
    ev = (_times(g, N), torch.full((N,), HOT[0]), torch.full((N,), HOT[1]), torch.randint(0, 2, (N,), generator=g).float())
    return ev, oracle_grid(ev, W, H, bins)


@functools.lru_cache(maxsize=None)
def ragged_case(sizes=(5000, 2, 777), bins=2, H=12, W=16):
    evs, refs = [], []
    for k, N in enumerate(sizes):
        g = torch.Generator().manual_seed(100 + k)
        ev = (_times(g, N), torch.rand(N, generator=g) * (W - 1), torch.rand(N, generator=g) * (H - 1),
              torch.randint(0, 2, (N,), generator=g).float())
        evs.append(ev)
        refs.append(oracle_grid(ev, W, H, bins) if N else torch.zeros(bins, H, W))
    return evs, refs


def _cat(evs):
    offsets = [0]
    for ev in evs:
        offsets.append(offsets[-1] + ev[0].numel())
    return [torch.cat([ev[k] for ev in evs]) for k in range(4)], offsets


def _golden(name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', name + '.npz')).items()}


# ------------------------------------------------------------------------------------------------------------------ voxel grid
@pytest.mark.parametrize('bins', [1, 5])
def test_voxel_ordered_dense_cells_bitwise(tgt, bins):
    """~100 contributions per cell (400 per cell at bins = 1): every cell goes through the workgroup sort in LDS"""
    ev, ref = dense_case(bins)
    got = ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], bins, 12, 16)
    assert got.shape == (bins, 12, 16)
    assert torch.equal(got.cpu(), ref), f'{int((got.cpu() != ref).sum())} of {ref.numel()} cells differ from the sequential sum'


def test_voxel_ordered_sparse_cells_bitwise(tgt):
    """the events of tests/golden/voxel.npz (48 x 64, ~0.4 .. 6 contributions per cell): the one-lane path"""
    g = _golden('voxel')
    for bins in (1, 5):
        ev = [g[f'{k}{bins}'] for k in 'txyp']
        got = ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], bins, 48, 64)
        assert torch.equal(got.cpu(), oracle_grid(ev, 64, 48, bins)), f'bins {bins}'
        assert_close(got, g[f'vg{bins}'], 2e-6, atol=1e-6, name='voxel grid (the bound of test_voxel_golden)')


def test_voxel_ordered_hot_pixel_bitwise(tgt):
    """all 8192 events on one pixel, 3 bins: 12 cells with segments of several thousand records, on either side of the LDS capacity"""
    ev, ref = hot_case(8192, 3)
    assert int((ref != 0).sum()) == 12
    got = ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], 3, 12, 16)
    assert torch.equal(got.cpu(), ref)


def test_voxel_ordered_segment_beyond_lds_bitwise(tgt):
    """four cells of 60 000 contributions each (480 KB of records per cell): the workgroup sort in global memory"""
    ev, ref = hot_case(60000, 1)
    assert int((ref != 0).sum()) == 4
    got = ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], 1, 12, 16)
    assert torch.equal(got.cpu(), ref)


def test_voxel_ordered_borders_bitwise(tgt):
    H, W, bins = 6, 8, 3
    g = torch.Generator().manual_seed(5)
    N = 96
    x = torch.rand(N, generator=g) * (W - 1)
    y = torch.rand(N, generator=g) * (H - 1)
    x[0:8] = W - 0.5                                     # the +1 column falls outside
    y[8:16] = H - 0.5                                    # the +1 row falls outside
    x[16:24] = -torch.rand(8, generator=g) * 0.98 - 0.01   # x in (-1, 0): truncates to column 0
    y[20:28] = -torch.rand(8, generator=g) * 0.98 - 0.01
    x[28:32] = torch.tensor([W, W + 0.3, W + 7.0, W + 0.999])   # fully masked
    y[32:36] = torch.tensor([H, H + 0.3, H + 7.0, H + 0.999])
    x[36:40], y[36:40] = W - 0.5, H - 0.5                # both at once
    x[-1], y[-1] = 2.25, 3.5                             # the last event sits in the last time bin: its +1 neighbour is masked
    ev = (_times(g, N), x, y, torch.randint(0, 2, (N,), generator=g).float())
    ref = oracle_grid(ev, W, H, bins)
    assert ref[bins - 1, 3, 2] != 0
    got = ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], bins, H, W)
    assert torch.equal(got.cpu(), ref)
    # one time bin: every event's +1 time neighbour is masked
    assert torch.equal(ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], 1, H, W).cpu(), oracle_grid(ev, W, H, 1))


def test_voxel_ordered_ragged_batch(tgt):
    evs, refs = ragged_case()
    cat, offsets = _cat(evs)
    got = ops.events_voxel_ordered_batch(*[tgt.to(a) for a in cat], offsets, 2, 12, 16)
    assert got.shape == (3, 2, 12, 16)
    for b, (ev, ref) in enumerate(zip(evs, refs)):
        single = ops.events_to_voxel_grid_ordered(*[tgt.to(a) for a in ev], 2, 12, 16)
        assert torch.equal(got[b].cpu(), ref), f'sample {b} against the oracle'
        assert torch.equal(got[b], single), f'sample {b} against the single-sample call'
    # an empty sample in the middle: zeros, and its neighbours do not move
    evs0, refs0 = ragged_case(sizes=(5000, 0, 777))
    cat, offsets = _cat(evs0)
    assert offsets == [0, 5000, 5000, 5777]
    got0 = ops.events_voxel_ordered_batch(*[tgt.to(a) for a in cat], offsets, 2, 12, 16)
    assert torch.equal(got0[1].cpu(), torch.zeros(2, 12, 16))
    assert torch.equal(got0[0], got[0]) and torch.equal(got0[2], got[2])
    # no events at all
    e = tgt.to(torch.zeros(0))
    assert torch.equal(ops.events_to_voxel_grid_ordered(e, e, e, e, 2, 12, 16).cpu(), torch.zeros(2, 12, 16))


# ------------------------------------------------------------------------------------------------------------------ event prep
def test_event_prep_batch_bitwise(tgt):
    H, W = 20, 30
    g = torch.Generator().manual_seed(11)
    raws = []
    for N in (700, 2, 0, 1300):
        raws.append((torch.sort(torch.randint(0, 50000, (N,), generator=g))[0] + 1_000_000 * (len(raws) + 1),
                     torch.randint(0, W, (N,), generator=g, dtype=torch.int32), torch.randint(0, H, (N,), generator=g, dtype=torch.int32),
                     torch.randint(0, 2, (N,), generator=g, dtype=torch.uint8)))
    raws[1] = (torch.tensor([5, 9]), raws[1][1], raws[1][2], raws[1][3])   # two distinct time stamps
    rect = torch.rand(H, W, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    cat, offsets = _cat(raws)
    for rm in (None, tgt.to(rect)):
        got = pl.event_prep_batch(*[tgt.to(a) for a in cat], offsets, rm, H, W)
        for b, raw in enumerate(raws):
            if raw[0].numel() == 0:
                continue
            want = pl.event_prep(*[tgt.to(a) for a in raw], rm, H, W)
            for name, a, w in zip(('t_norm', 'x', 'y', 'pol'), got, want):
                assert torch.equal(a[offsets[b]:offsets[b + 1]], w), f'sample {b}, {name}, rectify map: {rm is not None}'


# ------------------------------------------------------------------------------------------------------------------ events_norm
def test_events_norm_batch(tgt):
    """against the oracle within the bound tests/test_pipeline.py uses for the normalised grid; bit-identical from call to call"""
    grids = torch.stack([dense_case(5)[1], dense_case(5)[1].flip(0) * 0.5, torch.zeros(5, 12, 16)])
    clips = [0.9, 2.5, 1.0]
    dev_grids = tgt.to(grids)
    got = ops.events_norm_batch(dev_grids, clips)
    for b in range(3):
        assert_close(got[b], ouda.events_norm(grids[b].clone(), clips[b]), 1e-5, atol=1e-6, name=f'events_norm_batch, sample {b}')
    assert torch.equal(ops.events_norm_batch(dev_grids, clips), got), 'two calls on the same input differ'
    # a grid without events is not standardised (the reference's num_nonzeros == 0 branch passes it through unchanged); the
    # reference's two min-max normalisations then map the constant to -final_range, exactly as ops.events_norm does
    assert torch.equal(got[2], ops.events_norm(dev_grids[2], clips[2])) and bool(torch.isfinite(got[2]).all())
    # more than one statistics partial per grid (48 x 64 x 5 elements), another final range
    g = _golden('voxel')
    big = tgt.to(torch.stack([g['vg5'], g['vg5'] * 3]))
    clip = (5000 / 500000) * 1.5 * 100
    nrm = ops.events_norm_batch(big, [clip, clip])
    assert_close(nrm[0], g['norm5'], 1e-5, name='events_norm_batch against the golden fixture (the bound of test_voxel_golden)')
    assert_close(ops.events_norm_batch(big, [clip, 0.7], final_range=2.0)[1], ouda.events_norm(g['vg5'] * 3, 0.7, 2.0), 1e-5, atol=1e-6,
                 name='final_range 2')
    assert torch.equal(ops.events_norm_batch(big, [clip, clip]), nrm)


# ------------------------------------------------------------------------------------------------------------------ pipeline, dataset
def test_dsec_target_sample_ordered_golden(tgt):
    """the whole event branch (prep -> ordered grid -> norm -> crop / flip / resize) against the dsec-target fixture.  The default
    path cannot be held to this end to end (tests/test_pipeline.py pins its two stages separately: a cell that cancels to ~1e-8
    under one summation order and to 0 under another moves the non-zero count); the ordered grid is the reference's bit for bit."""
    g = {k: v for k, v in np.load(os.path.join(HERE, 'golden', 'pipeline.npz')).items()}
    dev = tgt.device
    frame = torch.from_numpy(g['t_frame'])[None].to(dev)
    events = [tuple(torch.from_numpy(g[k]).to(dev) for k in ('t_t', 't_x', 't_y', 't_p'))]
    rect = torch.from_numpy(g['t_rect']).to(dev)
    isr = dict(val_range=[0.01, 1.01], _threshold=0.005, _clip_range=0.1, shift_pixel=1)
    clip = (events[0][0].numel() - 1) / 500000 * 1.5 * 100
    for tag, direction in (('a', 'rightdown'), ('b', 'leftup')):
        x, y, flip = [int(v) for v in g[f't_{tag}_params']]
        out = pl.dsec_target_sample(frame, events, rect, [x], [y], [flip], isr, direction, crop=(40, 40), out_size=(52, 52),
                                    events_bins=1, events_clip_range=clip, ordered_events=True)
        assert_close(out['events_vg'][0], torch.from_numpy(g[f't_{tag}_events_vg']), 1e-6, atol=1e-6, name=f'events_vg ({tag})')
        base = pl.dsec_target_sample(frame, events, rect, [x], [y], [flip], isr, direction, crop=(40, 40), out_size=(52, 52),
                                     events_bins=1, events_clip_range=clip)
        assert torch.equal(out['warp_image'], base['warp_image']) and torch.equal(out['warp_img_self_res'], base['warp_img_self_res'])


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_dsec_dataset_ordered_events(tgt, mode):
    outputs = {'warp_image', 'events_vg', 'warp_img_self_res'} if mode == 'train' else {'warp_image', 'events_vg', 'label'}
    cfg = dict(type='DSECDataset', crop_size=(400, 400), after_crop_resize_size=(64, 64), events_bins=1, outputs=outputs,
               events_clip_range=(0.8, 1.2), synthetic_length=4, synthetic_events=3000, device=tgt.device)

    def batch(ordered):
        ds = D.build_dataset(dict(cfg, ordered_events=ordered))
        random.seed(7)
        out = ds.get_batch([1, 3])
        return out, random.random()

    (a, ra), (b, _), (base, rbase) = batch(True), batch(True), batch(False)
    assert torch.equal(a['events_vg'], b['events_vg']), 'ordered_events: events_vg differs between two identical runs'
    assert ra == rbase, 'the ordered path consumed other random draws than the default path'
    assert a['events_vg'].shape == base['events_vg'].shape
    assert_close(a['events_vg'], base['events_vg'], 1e-5, atol=1e-6, name='ordered against the default path')
    assert set(a) == set(base)
    for k in set(a) - {'events_vg'}:
        assert torch.equal(a[k], base[k]), k


# ------------------------------------------------------------------------------------------------------------------ refusals
def _raw(name, *args):
    return getattr(L.lib(), name)(*args)


def test_fifth_table_refusals(tgt):
    """decided on the host before any launch or access: the >= 2^29 sample comes through the offsets alone, over 4-element buffers"""
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    SHAPE, UNSUPPORTED = -1, -4
    ev = tgt.to(torch.arange(4).float())
    grid = tgt.to(torch.full((2, 2, 3, 4), 7.0))
    scratch_grid = tgt.to(torch.zeros(2, 2, 3, 4))
    ws = tgt.to(torch.zeros(4096, dtype=torch.float64))
    p = L.ptr

    def offs(*v):
        return (i64 * len(v))(*v)

    def voxel(offsets, B=1, bins=2, H=3, W=4, t=ev, g=grid, w=ws):
        return _raw('cmdax5_voxel_ordered', p(t), p(ev), p(ev), p(ev), offsets, p(g), p(w), i32(B), i32(bins), i32(H), i32(W), None)

    assert voxel(offs(0, 4), g=scratch_grid) == 0
    for kw in (dict(bins=0), dict(H=0), dict(W=0), dict(W=-3), dict(B=0), dict(B=-1), dict(B=257)):
        assert voxel(offs(0, 4), **kw) == SHAPE, kw
    assert voxel(offs(0, 3, 2), B=2) == SHAPE, 'offsets that decrease'
    assert voxel(offs(0, -1), B=1) == SHAPE
    assert voxel(offs(1, 4), B=1) == SHAPE, 'offsets[0] is 0'
    assert voxel(offs(0, 1 << 29), B=1) == SHAPE, 'a sample of 2^29 events'
    assert voxel(offs(0, 2, 2 + (1 << 29)), B=2) == SHAPE
    assert voxel(offs(0, 4), bins=1 << 10, H=1 << 11, W=1 << 10) == SHAPE, 'cells >= 2^31'
    for kw in (dict(t=None), dict(g=None), dict(w=None)):
        assert voxel(offs(0, 4), **kw) == UNSUPPORTED, kw
    assert voxel(None) == UNSUPPORTED
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert torch.equal(grid.cpu(), torch.full((2, 2, 3, 4), 7.0)), 'a refused call wrote to the grid'

    raw = (tgt.to(torch.arange(4)), tgt.to(torch.zeros(4, dtype=torch.int32)), tgt.to(torch.zeros(4, dtype=torch.int32)),
           tgt.to(torch.zeros(4, dtype=torch.uint8)))
    outs = [tgt.to(torch.zeros(4)) for _ in range(4)]

    def prep(offsets, B=1, H=3, W=4, t=raw[0], o=outs[0]):
        return _raw('cmdax5_event_prep_batch', p(t), p(raw[1]), p(raw[2]), p(raw[3]), offsets, i32(B), None, i32(H), i32(W), p(o),
                    p(outs[1]), p(outs[2]), p(outs[3]), None)

    assert prep(offs(0, 4)) == 0
    for kw in (dict(B=0), dict(B=257), dict(H=0), dict(W=0)):
        assert prep(offs(0, 4), **kw) == SHAPE, kw
    assert prep(offs(0, 3, 2), B=2) == SHAPE and prep(offs(0, 1 << 29)) == SHAPE and prep(offs(2, 4)) == SHAPE
    assert prep(offs(0, 4), t=None) == UNSUPPORTED and prep(offs(0, 4), o=None) == UNSUPPORTED and prep(None) == UNSUPPORTED

    clips = (f32 * 2)(1.0, 1.0)

    def norm(B=2, n=24, e=grid, o=grid, w=ws, c=clips):
        return _raw('cmdax5_events_norm_batch', p(e), p(o), p(w), i32(B), i64(n), c, f32(1.0), None)

    for kw in (dict(B=0), dict(B=257), dict(n=0), dict(n=1 << 31)):
        assert norm(**kw) == SHAPE, kw
    for kw in (dict(e=None), dict(o=None), dict(w=None), dict(c=None)):
        assert norm(**kw) == UNSUPPORTED, kw
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert torch.equal(grid.cpu(), torch.full((2, 2, 3, 4), 7.0))
    # the Python layer reports a refusal as an error
    with pytest.raises(L.CmdaError, match='bad shape'):
        ops.events_voxel_ordered_batch(ev, ev, ev, ev, [0, 4], 0, 3, 4)
    with pytest.raises(L.CmdaError, match='bad shape'):
        ops.events_voxel_ordered_batch(ev, ev, ev, ev, [0, 3, 2], 2, 3, 4)
