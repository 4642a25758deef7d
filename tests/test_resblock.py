"""Kernel-level tests of the eighth ABI table (include/cmda_hip_ext8.h, csrc/resblock.hip and cmdax8_bn_stats in csrc/batchnorm.hip)
against float64 written out here, on the stored inputs (bf16 values widened).

Inputs per branch: z ~ 2 N(0, 1) + 1 (+ 7 g in group g), mean ~ 0.5 N + 1 (+ 7 g), rstd and gamma uniform in [0.5, 1.5], beta ~ 0.2 N;
x = t - bn64(z) rounded to the storage type with |t| uniform in [0.25, 2] and a random sign, so the pre-activation bn(z) + x is t up to
the rounding of x.  Every case asserts, in float64, that no pre-activation lies within 0.1 of zero: no ReLU mask can flip, and no
outlier allowance is used anywhere.

Bounds (the project's own, tests/test_kernels.py): forward 3e-5 of the tensor's maximum in fp32, 4e-3 with bf16 storage (one rounding
of the result, 2^-9 = 2e-3 of the element); dz / dres twice that; dgamma / dbeta, added onto non-zero starting values, 1e-4.
"""
import ctypes

import pytest
import torch

from cmda_amd import _lib, ops
from conftest import assert_close, check_ge, check_le

DT = [(torch.float32, 3e-5), (torch.bfloat16, 4e-3)]
SHAPES = [(1, 4, 1), (2, 8, 2), (15, 64, 1), (515, 320, 2), (1024, 64, 2), (4099, 512, 1)]
MULTI = [(1024, 64), (256, 128), (64, 320), (15, 512)]
_BN_COND_K = 20.5   # tests/test_kernels.py: the conditioning constant of the one-pass variance


def _branch(M, C, G, dt, gen):
    """stored inputs of one branch and the float64 pre-activation / xhat [G, M, C]"""
    off = 7.0 * torch.arange(G, dtype=torch.float32)
    z = (torch.randn(G, M, C, generator=gen) * 2 + 1 + off.view(G, 1, 1)).to(dt)
    mean = torch.randn(G, C, generator=gen) * 0.5 + 1 + off.view(G, 1)
    rstd = torch.rand(G, C, generator=gen) + 0.5
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.2
    xhat = (z.double() - mean.double()[:, None]) * rstd.double()[:, None]
    bn = xhat * gamma.double() + beta.double()
    t = (torch.rand(G, M, C, generator=gen, dtype=torch.float64) * 1.75 + 0.25) * (torch.randint(0, 2, (G, M, C), generator=gen) * 2 - 1)
    x = (t - bn).to(dt)
    pre = bn + x.double()
    return dict(z=z, x=x, mean=mean, rstd=rstd, gamma=gamma, beta=beta, xhat=xhat, pre=pre)


def _level(M, C, G, dt, gen):
    """one level: two branches, dout, non-zero starting dgamma / dbeta, and the float64 results"""
    lv = dict(M=M, C=C, br=[_branch(M, C, G, dt, gen) for _ in range(2)])
    lv['dout'] = torch.randn(G, M, C, generator=gen).to(dt)
    margin = min(b['pre'].abs().min().item() for b in lv['br'])
    check_ge('smallest |pre-activation| in float64', margin, 0.1)
    lv['out64'] = 0.5 * (lv['br'][0]['pre'].clamp(min=0) + lv['br'][1]['pre'].clamp(min=0))
    for b in lv['br']:
        g = 0.5 * lv['dout'].double() * (b['pre'] > 0)
        s1, s2 = g.sum(1), (g * b['xhat']).sum(1)
        b['dz64'] = (b['gamma'].double() * b['rstd'].double()[:, None]) * (g - s1[:, None] / M - b['xhat'] * s2[:, None] / M)
        b['dres64'] = g
        b['dg0'], b['db0'] = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        b['dgamma64'], b['dbeta64'] = b['dg0'].double() + s2.sum(0), b['db0'].double() + s1.sum(0)
    return lv


def _device_level(tgt, lv, G, backward, out=None):
    M, C = lv['M'], lv['C']
    d = dict(M=M, C=C)
    for name, b in zip(('image', 'events'), lv['br']):
        d[name] = dict(z=tgt.to(b['z'].view(G * M, C)), x=tgt.to(b['x'].view(G * M, C)), mean=tgt.to(b['mean']), rstd=tgt.to(b['rstd']),
                       gamma=tgt.to(b['gamma']), beta=tgt.to(b['beta']))
        if backward:
            d[name].update(dgamma=tgt.to(b['dg0'].clone()), dbeta=tgt.to(b['db0'].clone()))
    if backward:
        d['dout'] = tgt.to(lv['dout'].view(G * M, C))
    else:
        d['out'] = out
    return d


def _run_and_check(tgt, dt, tol, shapes, G, seed):
    gen = torch.Generator().manual_seed(seed)
    lvs = [_level(M, C, G, dt, gen) for M, C in shapes]
    # forward: every output is the middle row slice of a NaN-filled buffer three times its size
    bufs = [torch.full((3 * G * lv['M'], lv['C']), float('nan'), dtype=dt, device=tgt.device) for lv in lvs]
    outs = [buf[G * lv['M']:2 * G * lv['M']] for buf, lv in zip(bufs, lvs)]
    ops.resavg_fwd([_device_level(tgt, lv, G, False, out) for lv, out in zip(lvs, outs)], G)
    for i, (lv, buf) in enumerate(zip(lvs, bufs)):
        n = G * lv['M']
        assert_close(buf[n:2 * n], lv['out64'].view(n, -1), tol, name=f'level {i} out')
        assert torch.isnan(buf[:n]).all().item() and torch.isnan(buf[2 * n:]).all().item(), 'rows outside the slice were written'
    # backward
    devs = [_device_level(tgt, lv, G, True) for lv in lvs]
    grads = ops.resavg_bwd(devs, G)
    for i, (lv, dev, pairs) in enumerate(zip(lvs, devs, grads)):
        n = G * lv['M']
        for name, b, (dz, dres) in zip(('image', 'events'), lv['br'], pairs):
            assert_close(dz, b['dz64'].view(n, -1), 2 * tol, name=f'level {i} {name} dz')
            assert_close(dres, b['dres64'].view(n, -1), 2 * tol, name=f'level {i} {name} dres')
            assert_close(dev[name]['dgamma'], b['dgamma64'], 1e-4, name=f'level {i} {name} dgamma')
            assert_close(dev[name]['dbeta'], b['dbeta64'], 1e-4, name=f'level {i} {name} dbeta')
    return lvs


@pytest.mark.parametrize('dt,tol', DT)
@pytest.mark.parametrize('M,C,G', SHAPES)
def test_resavg_against_float64(tgt, dt, tol, M, C, G):
    """cmdax8_resavg_fwd / cmdax8_resavg_bwd, one level: M = 1 / 2, fewer rows than a block sweeps per iteration (its row lanes x the unroll), a ragged tail
    with C over more than one column block, several row blocks per group, groups with their own statistics; the output written into
    a row slice of a NaN-filled buffer"""
    _run_and_check(tgt, dt, tol, [(M, C)], G, seed=M + C + G)


@pytest.mark.parametrize('dt,tol', DT)
def test_resavg_four_levels_one_grid(tgt, dt, tol):
    """one call for four levels of different M and C with groups=2: the level boundaries fall inside one grid"""
    _run_and_check(tgt, dt, tol, MULTI, 2, seed=77)


@pytest.mark.parametrize('dt,tol', DT)
def test_resavg_groups_use_their_own_statistics(tgt, dt, tol):
    """groups=2 with group means 7 apart (3.5 standard deviations of z, as tests/test_kernels.py::_bn_inputs): the grouped call equals
    two one-group calls on the halves, and statistics row 0 applied to group 1 is visibly wrong"""
    M, C, G = 64, 32, 2
    gen = torch.Generator().manual_seed(5)
    lv = _level(M, C, G, dt, gen)
    out = torch.empty(G * M, C, dtype=dt, device=tgt.device)
    ops.resavg_fwd([_device_level(tgt, lv, G, False, out)], G)
    for g in range(G):
        half = dict(M=M, C=C, br=[{k: (v[g:g + 1] if k in ('z', 'x', 'mean', 'rstd') else v) for k, v in b.items()} for b in lv['br']])
        o = torch.empty(M, C, dtype=dt, device=tgt.device)
        ops.resavg_fwd([_device_level(tgt, half, 1, False, o)], 1)
        assert torch.equal(o.cpu(), out[g * M:(g + 1) * M].cpu()), f'group {g}'
    wrong = [dict(b, mean=b['mean'][:1].expand(G, C).contiguous(), rstd=b['rstd'][:1].expand(G, C).contiguous()) for b in lv['br']]
    o = torch.empty(G * M, C, dtype=dt, device=tgt.device)
    ops.resavg_fwd([_device_level(tgt, dict(lv, br=wrong), G, False, o)], G)
    err = (o[M:].double().cpu() - lv['out64'][1]).abs().max().item() / lv['out64'][1].abs().max().item()
    check_ge('relative error of group 1 under group 0 statistics', err, 100 * tol)


# ---------------------------------------------------------------------------------------------- cmdax8_bn_stats
def _stats_case(tgt, dt, M, C, G, order, from_ws):
    eps, mom = 1e-5, 0.1
    gen = torch.Generator().manual_seed(M + C + G)
    x = (torch.randn(G, M, C, generator=gen) * 2 + 3 + 7.0 * torch.arange(G, dtype=torch.float32).view(G, 1, 1)).to(dt)
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    x64 = x.double()
    mean = x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps).rsqrt()
    rm, rv = rm0.double(), rv0.double()
    for g in (order or range(G)):
        rm = (1 - mom) * rm + mom * mean[g]
        rv = (1 - mom) * rv + mom * var[g] * M / (M - 1)
    rmd, rvd = tgt.to(rm0.clone()), tgt.to(rv0.clone())
    ws = None
    if from_ws:
        # what a GEMM epilogue leaves (cmda_gemm colstats): per group 32 slots of [sum x | sum x^2] (no shift), the 33rd row unused
        slots = ops.L.lib().cmda_bn_ws_floats(C) // (2 * C) - 1
        assert slots == 32 and M % slots == 0
        parts = x64.view(G, slots, M // slots, C)
        ws = torch.zeros(G, slots + 1, 2 * C)
        ws[:, :slots, :C] = parts.sum(2).float()
        ws[:, :slots, C:] = (parts ** 2).sum(2).float()
        ws = tgt.to(ws.view(-1).contiguous())
    mean_k, rstd_k = ops.bn_stats(tgt.to(x.view(G * M, C)), rmd, rvd, M, C, eps, mom, G, order, stats_ws=ws)
    assert_close(mean_k, mean, 1e-5, name='mean')
    # tests/test_kernels.py::_bn_train_case: 1e-5 plus the channel's conditioning term, the variance being taken in one pass around the
    # shift (row 0 of the group; 0 for epilogue sums)
    shift = torch.zeros_like(mean) if from_ws else x64[:, 0]
    kappa = 1 + (mean - shift) ** 2 / var
    bound = 1e-5 + _BN_COND_K / 2 * 2.0 ** -24 * kappa
    check_le('rstd: relative error / (1e-5 + K/2 2^-24 kappa)', ((rstd_k.double().cpu() - rstd).abs() / rstd / bound).max().item(), 1.0)
    assert_close(rmd, rm, 1e-5, name='running_mean')
    assert_close(rvd, rv, 1e-5, name='running_var')
    if from_ws:
        assert not ws.any().item(), 'the epilogue workspace must be handed back zeroed'
    if G > 1:   # `order` is honoured: the other order gives visibly different running statistics
        rm2 = rm0.double()
        for g in reversed(order or range(G)):
            rm2 = (1 - mom) * rm2 + mom * mean[g]
        check_ge('running_mean: distance between the two orders / 1e-5 bound', (rm2 - rm).abs().max().item() / rm.abs().max().item(), 1e-3)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('from_ws', [False, True], ids=['reduce', 'epilogue_ws'])
@pytest.mark.parametrize('M,C,G,order', [(515, 36, 1, None), (1024, 64, 2, (1, 0)), (256, 260, 3, (2, 0, 1))])
def test_bn_stats(tgt, dt, from_ws, M, C, G, order):
    """cmdax8_bn_stats against float64: saved mean / rstd per group, running statistics after the groups' updates in `order` (from
    non-trivial starting values), from its own reduction and from a filled epilogue workspace, which comes back zeroed"""
    if from_ws and M % 32:
        M = 512
    _stats_case(tgt, dt, M, C, G, order, from_ws)


# ---------------------------------------------------------------------------------------------- refusals
def test_eighth_table_refusals(tgt):
    """every refusal of cmda_hip_ext8.h returns its code and leaves NaN / sentinel-filled outputs untouched"""
    lib = ops.L.lib()
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    M, C, G = 8, 8, 1
    dev = tgt.device
    t = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    keep = dict(z=t(M, C), x=t(M, C), mean=t(G, C), rstd=t(G, C) + 1, gamma=t(C) + 1, beta=t(C))
    out = torch.full((M, C), float('nan'), device=dev)
    dz, dres = torch.full((M, C), float('nan'), device=dev), torch.full((M, C), float('nan'), device=dev)
    dg, db = torch.full((C,), 7.0, device=dev), torch.full((C,), 7.0, device=dev)
    dout = t(M, C) + 1
    ws = torch.full((4 * 33 * 2 * C,), 5.0, device=dev)

    def levels(n=1, **over):
        arr = (_lib.Level8 * max(n, 1))()
        for d in arr:
            for b in d.br:
                b.z, b.x, b.mean, b.rstd, b.gamma, b.beta = (keep[k].data_ptr() for k in ('z', 'x', 'mean', 'rstd', 'gamma', 'beta'))
                b.dz, b.dres, b.dgamma, b.dbeta = dz.data_ptr(), dres.data_ptr(), dg.data_ptr(), db.data_ptr()
            d.out, d.dout, d.M, d.C = out.data_ptr(), dout.data_ptr(), M, C
            for k, v in over.items():
                if k in ('M', 'C', 'out', 'dout'):
                    setattr(d, k, v)
                else:
                    setattr(d.br[1], k, v)
        return arr

    def both(arr, n=1, groups=1, dtype=0, wsp=None):
        wsp = ctypes.c_void_p(ws.data_ptr()) if wsp is None else wsp
        return (lib.cmdax8_resavg_fwd(arr, i32(n), i32(groups), i32(dtype), None),
                lib.cmdax8_resavg_bwd(arr, i32(n), i32(groups), wsp, i32(dtype), None))

    def bwd_only(arr):   # (pointers the forward entry does not read: it would run)
        return lib.cmdax8_resavg_bwd(arr, i32(1), i32(1), ctypes.c_void_p(ws.data_ptr()), i32(0), None)

    SHAPE, DTYPE, UNSUP = -1, -2, -4
    assert both(levels(C=6)) == (SHAPE, SHAPE) and both(levels(C=0)) == (SHAPE, SHAPE)
    assert both(levels(), n=0) == (SHAPE, SHAPE) and both(levels(5), n=5) == (SHAPE, SHAPE)
    assert both(levels(), groups=0) == (SHAPE, SHAPE) and both(levels(), groups=9) == (SHAPE, SHAPE)
    assert both(levels(M=0)) == (SHAPE, SHAPE)
    assert both(levels(M=2 ** 31 // 8)) == (SHAPE, SHAPE)              # groups*M*C = 2^31
    assert both(levels(M=2 ** 31 // 16), groups=2) == (SHAPE, SHAPE)
    assert both(levels(), dtype=2) == (DTYPE, DTYPE) and both(levels(), dtype=-1) == (DTYPE, DTYPE)
    for k in ('z', 'x', 'mean', 'rstd', 'gamma', 'beta'):
        assert both(levels(**{k: None})) == (UNSUP, UNSUP), k
    assert lib.cmdax8_resavg_fwd(levels(out=None), i32(1), i32(1), i32(0), None) == UNSUP
    assert lib.cmdax8_resavg_fwd(None, i32(1), i32(1), i32(0), None) == UNSUP
    for k in ('dz', 'dres', 'dgamma', 'dbeta'):
        assert bwd_only(levels(**{k: None})) == UNSUP, k
    assert bwd_only(levels(dout=None)) == UNSUP
    assert lib.cmdax8_resavg_bwd(levels(), i32(1), i32(1), None, i32(0), None) == UNSUP
    # the workspace query follows the same shape rules
    assert lib.cmdax8_ws_floats(levels(), 1, 1) == 2 * 33 * 2 * C and lib.cmdax8_ws_floats(levels(2), 2, 3) == 2 * 2 * 3 * 33 * 2 * C
    assert lib.cmdax8_ws_floats(levels(C=6), 1, 1) == -1 and lib.cmdax8_ws_floats(levels(), 0, 1) == -1
    assert lib.cmdax8_ws_floats(levels(), 1, 9) == -1 and lib.cmdax8_ws_floats(None, 1, 1) == -1
    # the statistics entry: cmda_bn_train_fwd's refusals
    mean, rstd = torch.full((2, C), float('nan'), device=dev), torch.full((2, C), float('nan'), device=dev)
    rmv = torch.full((C,), 3.0, device=dev)

    def stats(C_=C, groups=1, order=None, has=0, dtype=0):
        oc = (ctypes.c_int * len(order))(*order) if order else None
        return lib.cmdax8_bn_stats(ctypes.c_void_p(keep['z'].data_ptr()), ctypes.c_void_p(mean.data_ptr()), ctypes.c_void_p(rstd.data_ptr()),
                                   ctypes.c_void_p(rmv.data_ptr()), ctypes.c_void_p(rmv.data_ptr()), ctypes.c_void_p(ws.data_ptr()), i64(4),
                                   i32(C_), f32(1e-5), f32(0.1), i32(groups), oc, i32(has), i32(dtype), None)
    assert stats(C_=6) == SHAPE and stats(groups=0) == SHAPE and stats(groups=9) == SHAPE
    assert stats(groups=2, order=(0, 2)) == SHAPE and stats(groups=2, order=(1, 1), has=1) == SHAPE
    assert stats(dtype=3) == DTYPE
    # nothing was written by any refused call
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    for name, buf in (('out', out), ('dz', dz), ('dres', dres), ('mean', mean), ('rstd', rstd)):
        assert torch.isnan(buf).all().item(), name
    assert (dg == 7).all().item() and (db == 7).all().item() and (ws == 5).all().item() and (rmv == 3).all().item()
