"""The dilated depthwise kernels of dwconv.hip (the sep-ASPP branches) at every launch regime, against float64 F.conv2d on the CPU.

  1. exact arithmetic: integer-valued inputs make every fp32 accumulation order exact, so y, the BatchNorm statistics, dx, dx
     accumulated onto a previous gradient, dweight and dbias are compared with torch.equal -- no tolerance.  Each case asserts, from a
     restatement of the launch geometry, the regime it was written for (ring wrap, channel groups, statistics groups inside one
     workgroup, slot wrap, weight-gradient block shape), so a later edit of a shape cannot silently leave it;
  2. real-valued inputs on the same paths: integers never round, so this part holds the rounding to a derived elementwise bound;
  3. dilation with GELU (the row-run stencils: forward, backward prep, fused backward) at test_kernels.test_dwconv's tolerances;
  4. what the entry points refuse, at the C ABI.
The dilation-1 row walk is tests/test_dwconv_walk.py's."""
import functools

import pytest
import torch
import torch.nn.functional as F

from cmda_amd import _lib as L
from cmda_amd import ops
from conftest import assert_close, check_le

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id='bf16'), pytest.param(FP32, id='fp32')]

# ---- the launch geometry of dwconv.hip, restated (names: the constants they mirror)
DRUN = 4                    # DRUN: sub-columns per thread of dw_dilated_walk
WALK_QUADS = 64             # launch_stencil's `cq`: channel quads per workgroup of dw_dilated_kernel; 256 / 64 = 4 run lanes
WGRAD_QUADS = 16            # cmda_dwconv3x3_bwd_weight's `cq`: channel quads per workgroup of dw_bwd_weight_kernel; 16 run lanes
RUN_LEN = {BF16: 8, FP32: 4}   # RunLen<T>::value: outputs per run of the row-run kernels
BN_SLOTS = 32               # CMDA_BN_SLOTS: slots per group of the BatchNorm workspace (+ 1 that the finishing pass owns)
WGRAD_MIN_BLOCKS = 768      # cmda_dwconv3x3_bwd_weight: the grid below which k is halved


def _cdiv(a, b):
    return -(-a // b)


def walk_geom(B, H, W, C, dil):
    """dw_dilated_kernel: thread t -> (image, rho_h, rho_w, run k), k fastest; a workgroup holds 4 consecutive t x 64 channel quads"""
    rpc = _cdiv(_cdiv(W, dil), DRUN)
    lanes = 256 // WALK_QUADS
    run_blocks = _cdiv(B * dil * dil * rpc, lanes)
    gx = _cdiv(C // 4, WALK_QUADS)
    return dict(rpc=rpc, per_image=dil * dil * rpc, lanes=lanes, run_blocks=run_blocks, gx=gx, grid=run_blocks * gx,
                nr=[max(0, _cdiv(H - r, dil)) for r in range(dil)], ncol=[max(0, _cdiv(W - r, dil)) for r in range(dil)])


def splits_a_workgroup(g, B, ipg):
    """a boundary between two statistics groups falls inside the 4 run lanes of one workgroup (`uniform == false`)"""
    return any((grp * ipg * g['per_image']) % g['lanes'] for grp in range(1, B // ipg))


def wgrad_k(B, H, W, C, dil, dt):
    """cmda_dwconv3x3_bwd_weight: runs per run lane"""
    rl = 256 // WGRAD_QUADS
    nruns = B * H * dil * _cdiv(_cdiv(W, dil), RUN_LEN[dt])
    gx = _cdiv(C // 4, WGRAD_QUADS)
    k = 8
    while k > 2 and _cdiv(nruns, rl * k) * gx < WGRAD_MIN_BLOCKS:
        k >>= 1
    return k


# ---- cases: (B, H, W, C, dil), images per group, the regimes the case exists for (asserted by _assert_regimes)
CASES = {
    'split': ((2, 7, 11, 8, 3), (1, 2), {'split'}),                       # 9 threads per image
    'split_gx2': ((3, 5, 4, 260, 3), (1, 3), {'split', 'gx', 'tail'}),    # ... and C = 4 * 65: one live quad in the second channel group
    'wrap_dil2': ((1, 23, 9, 12, 2), (1,), {'wrap'}),                     # 12 / 11 sub-rows: the ring of three wraps four times
    'head': ((2, 45, 30, 516, 6), (1, 2), {'wrap', 'gx', 'tail', 'slots', 'grid8', 'ragged'}),   # 8 / 7 sub-rows, gx = 3, 36 run blocks
    'odd_dil': ((4, 9, 40, 72, 5), (1, 2, 4), {'split', 'aligned', 'nr_differs'}),   # boundaries at t = 50, 100, 150
    'all_halo': ((1, 5, 7, 8, 12), (1,), {'single_pixel', 'empty'}),      # dilation above H and W
    'w_eq_dil': ((1, 9, 6, 8, 6), (1,), {'one_column'}),                  # W = dil: every sub-lattice one column, both halos padding
    'w_dil_plus_1': ((1, 9, 7, 8, 6), (1,), {'two_and_one_columns'}),     # W = dil + 1: residue 0 has two columns, the others one
    'ragged_32': ((1, 14, 75, 8, 4), (1,), {'wrap', 'ragged', 'ragged_mix'}),   # 5 runs per sub-row; 19 / 18 sub-columns
    'ragged_21': ((1, 9, 21, 8, 4), (1,), {'ragged', 'ragged_mix'}),      # 2 runs per sub-row; 6 / 5 sub-columns
}


def _assert_regimes(name):
    (B, H, W, C, dil), ipgs, regimes = CASES[name]
    g = walk_geom(B, H, W, C, dil)
    for r in regimes:
        if r == 'split':      # ipg = 1 puts a group boundary inside a workgroup
            assert g['per_image'] % g['lanes'] != 0 and B > 1 and 1 in ipgs
            assert splits_a_workgroup(g, B, 1)
        elif r == 'aligned':  # ... and another boundary between two workgroups, in the same launch
            assert any((grp * g['per_image']) % g['lanes'] == 0 for grp in range(1, B))
        elif r == 'wrap':
            assert max(g['nr']) > 3
        elif r == 'gx':
            assert g['gx'] > 1
        elif r == 'tail':     # the last channel group is not full
            assert g['gx'] > 1 and (C // 4) % WALK_QUADS != 0
        elif r == 'slots':
            assert g['run_blocks'] > BN_SLOTS
        elif r == 'grid8':
            assert g['gx'] > 1 and g['grid'] % 8 != 0
        elif r == 'ragged':   # several runs per sub-row, the last one short
            assert g['rpc'] > 1 and any(n % DRUN for n in g['ncol'])
        elif r == 'ragged_mix':
            assert len({n % DRUN for n in g['ncol']} - {0}) >= 2
        elif r == 'nr_differs':
            assert dil % 2 == 1 and len(set(g['nr'])) > 1
        elif r == 'single_pixel':
            assert dil > H and dil > W and max(g['nr']) == 1 and max(g['ncol']) == 1
        elif r == 'empty':
            assert min(g['nr']) == 0 and min(g['ncol']) == 0
        elif r == 'one_column':
            assert W == dil and set(g['ncol']) == {1}
        elif r == 'two_and_one_columns':
            assert W == dil + 1 and g['ncol'][0] == 2 and set(g['ncol'][1:]) == {1}
        else:
            raise AssertionError(r)
    return g


def test_regimes_of_the_case_table():
    """every regime the issue lists is claimed by some case (and each case asserts its own before it launches)"""
    for name in CASES:
        _assert_regimes(name)
    claimed = set().union(*(c[2] for c in CASES.values()))
    assert {'split', 'wrap', 'gx', 'tail', 'slots', 'grid8', 'ragged', 'single_pixel', 'empty'} <= claimed
    assert walk_geom(1, 128, 128, 1024, 6)['per_image'] % 4 == 0   # (the production shapes never split a workgroup)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ref64(x, w, dy, dil, bias=None, gelu=False):
    """float64 F.conv2d (+ erf GELU) and its autograd, from the inputs as the kernels see them -> z, y, dx, dw [C][9], dbias"""
    C = x.shape[-1]
    xr = _nchw(x).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = bias.double().requires_grad_(True) if bias is not None else None
    z = F.conv2d(xr, wr, br, padding=dil, dilation=dil, groups=C)
    y = F.gelu(z) if gelu else z
    y.backward(_nchw(dy))
    return (_nhwc(z.detach()), _nhwc(y.detach()), _nhwc(xr.grad), wr.grad.reshape(C, 9), br.grad if bias is not None else None)


def _tap_major(w):
    return w.reshape(w.shape[0], 9).t().contiguous()   # [9][C], what the kernels read


def _read_stats(ws, G, C):
    """as test_kernels.test_dwconv reads them, in float64; slot 32 belongs to the finishing pass and stays zero"""
    v = ws.view(G, BN_SLOTS + 1, 2, C).cpu().double()
    assert v[:, BN_SLOTS].abs().max().item() == 0, 'slot 32 of the BatchNorm workspace was written'
    return v[:, :BN_SLOTS].sum(1)


def _new_ws(tgt, G, C):
    return torch.zeros(G * int(L.lib().cmda_bn_ws_floats(C)), device=tgt.device)


# ====================================================================================================== 1. exact arithmetic
@functools.lru_cache(maxsize=None)
def _exact_case(name):
    """integer-valued inputs (the same in bf16 and fp32) and their float64 reference, computed once and never written to"""
    (B, H, W, C, dil), _, _ = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    x, dy, prev = ri(-3, 3, B, H, W, C), ri(-3, 3, B, H, W, C), ri(-9, 9, B, H, W, C)
    w, bias = ri(-2, 2, C, 1, 3, 3), ri(-2, 2, C)
    _, y, dx, dw, _ = _ref64(x, w, dy, dil)
    return dict(x=x, dy=dy, prev=prev, w=w, bias=bias, y=y, dx=dx, dw=dw, db=dy.double().sum((0, 1, 2)),
                dw_abs=_ref64(x.abs(), w, dy.abs(), dil)[3])


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(CASES))
def test_exact(tgt, dt, name):
    (B, H, W, C, dil), ipgs, _ = CASES[name]
    _assert_regimes(name)
    c = _exact_case(name)
    y, dx, dw, db = c['y'], c['dx'], c['dw'], c['db']
    # exactness is a precondition, asserted on the reference alone
    acc_ref, yb_ref = dx + c['prev'].double(), y + c['bias'].double()
    assert max(t.abs().max().item() for t in (y, yb_ref, dx, acc_ref)) <= 256
    assert c['dw_abs'].max().item() + 1 < 2 ** 24 and c['dy'].abs().sum((0, 1, 2)).max().item() + 1 < 2 ** 24
    for ipg in ipgs:
        yg = y.reshape(B // ipg, ipg * H * W, C)
        assert yg.abs().sum(1).max().item() < 2 ** 24 and (yg * yg).sum(1).max().item() < 2 ** 24

    xd, dyd, wd = tgt.to(c['x'].to(dt)), tgt.to(c['dy'].to(dt)), tgt.to(_tap_major(c['w']))
    got = ops.dwconv_fwd(xd, wd, None, B, H, W, C, dil, None)
    assert got.dtype == dt and torch.equal(got.cpu().double(), y), 'forward'
    got_b = ops.dwconv_fwd(xd, wd, tgt.to(c['bias']), B, H, W, C, dil, None)
    assert torch.equal(got_b.cpu().double(), yb_ref), 'forward with bias'
    for ipg in ipgs:
        G = B // ipg
        ws = _new_ws(tgt, G, C)
        y2 = ops.dwconv_fwd(xd, wd, None, B, H, W, C, dil, None, colstats=(ws, ipg))
        assert torch.equal(y2, got), f'forward with statistics, {ipg} images per group: y differs from the plain call'
        st = _read_stats(ws, G, C)
        yg = y.reshape(G, ipg * H * W, C)
        assert torch.equal(st[:, 0], yg.sum(1)), f'column sums, {ipg} images per group'
        assert torch.equal(st[:, 1], (yg * yg).sum(1)), f'column sums of squares, {ipg} images per group'
    got = ops.dwconv_bwd_data(dyd, wd, B, H, W, C, dil)
    assert torch.equal(got.cpu().double(), dx), 'dx'
    got = ops.dwconv_bwd_data(dyd, wd, B, H, W, C, dil, out=tgt.to(c['prev'].to(dt)), accumulate=True)
    assert torch.equal(got.cpu().double(), acc_ref), 'dx accumulated'
    assert wgrad_k(B, H, W, C, dil, dt) == 2
    dwd, dbd = torch.ones(C, 9, device=tgt.device), torch.ones(C, device=tgt.device)   # 1: they are added to
    ops.dwconv_bwd_weight(dyd, xd, dwd, dbd, B, H, W, C, dil)
    assert torch.equal(dwd.cpu().double(), dw + 1), 'dweight'
    assert torch.equal(dbd.cpu().double(), db + 1), 'dbias'
    dwd = torch.ones(C, 9, device=tgt.device)
    ops.dwconv_bwd_weight(dyd, xd, dwd, None, B, H, W, C, dil)
    assert torch.equal(dwd.cpu().double(), dw + 1), 'dweight without dbias'


# the weight gradient's block shapes: k runs per run lane, 8 at the decode head's sizes; C = 1024 is the head's 16 channel groups
WGRAD_CASES = {4: (1, 1536, 4, 1024, 2), 8: (1, 3072, 4, 1024, 2)}


@functools.lru_cache(maxsize=None)
def _wgrad_case(k):
    B, H, W, C, dil = WGRAD_CASES[k]
    gen = torch.Generator().manual_seed(k)
    x = torch.randint(-3, 4, (B, H, W, C), generator=gen).float()
    dz = torch.randint(-3, 4, (B, H, W, C), generator=gen).float()
    w = torch.zeros(C, 1, 3, 3)   # (dweight does not depend on it)
    # sum |dz x| per (channel, tap) <= pixels * max |dz| * max |x|: the exactness precondition without a second 12 M-element pass
    return dict(x=x, dz=dz, dw=_ref64(x, w, dz, dil)[3], dw_abs_bound=B * H * W * dz.abs().max().item() * x.abs().max().item(),
                db=dz.double().sum((0, 1, 2)))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('k', [4, 8])
def test_exact_weight_gradient_block_shapes(tgt, dt, k):
    B, H, W, C, dil = WGRAD_CASES[k]
    assert wgrad_k(B, H, W, C, dil, dt) == k
    assert _cdiv(C // 4, WGRAD_QUADS) > 1
    c = _wgrad_case(k)
    assert c['dw_abs_bound'] + 1 < 2 ** 24 and c['dz'].abs().sum((0, 1, 2)).max().item() + 1 < 2 ** 24
    dwd, dbd = torch.ones(C, 9, device=tgt.device), torch.ones(C, device=tgt.device)
    ops.dwconv_bwd_weight(tgt.to(c['dz'].to(dt)), tgt.to(c['x'].to(dt)), dwd, dbd, B, H, W, C, dil)
    assert torch.equal(dwd.cpu().double(), c['dw'] + 1), 'dweight'
    assert torch.equal(dbd.cpu().double(), c['db'] + 1), 'dbias'


# ====================================================================================================== 2. real-valued inputs
# |got - ref| <= r |ref| + 16 * 2^-24 * A elementwise, A = the same convolution of the absolute values (+ |prev| when accumulating).
# A stencil sum is ten fp32 operations (nine taps and the previous value): at most gamma_10 * A, the 16 is margin over the 10;
# r = 2^-8 is bf16's half ulp under round-to-nearest-even, r = 0 for fp32 storage -- truncation (2^-7) fails.  dweight / dbias and the
# statistics are fp32 whatever the storage (r = 0).  They are sums of N <= 2700 terms here, whose worst case would be gamma_N * A; the
# same 16 * 2^-24 * A is applied to them as well: A grows with N and the rounding of a sum of N terms of either sign with sqrt(N).
# Statistics: the sum as above; for the sum of squares (y + e)^2 - y^2 = 2 y e + e^2 with |e| <= gamma_10 A, and the square rounds
# once more (A >= |y|): 32 * 2^-24 * sum(A |y|).
U24 = 2.0 ** -24
REAL_CASES = ['head', 'wrap_dil2', 'split']


@functools.lru_cache(maxsize=None)
def _real_case(name, dt):
    (B, H, W, C, dil), _, _ = CASES[name]
    gen = torch.Generator().manual_seed(17 + sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, dy, prev = rn(B, H, W, C).to(dt), rn(B, H, W, C).to(dt), rn(B, H, W, C).to(dt)
    w = 0.3 * rn(C, 1, 3, 3)
    _, y, dx, dw, _ = _ref64(x, w, dy, dil)
    _, ya, dxa, dwa, _ = _ref64(x.abs(), w.abs(), dy.abs(), dil)
    return dict(x=x, dy=dy, prev=prev, w=w, y=y, dx=dx, dw=dw, ya=ya, dxa=dxa, dwa=dwa)


def _check_bound(name, got, ref, A, r):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, name
    err, bound = (got - ref).abs(), r * ref.abs() + 16 * U24 * A
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)   # (err > 0 on a zero bound: inf)
    check_le(name + ' [worst |got - ref| / bound]', ratio.max().item(), 1.0)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', REAL_CASES)
def test_rounding(tgt, dt, name):
    (B, H, W, C, dil), ipgs, _ = CASES[name]
    _assert_regimes(name)
    c = _real_case(name, dt)
    r = 2.0 ** -8 if dt == BF16 else 0.0
    xd, dyd, wd = tgt.to(c['x']), tgt.to(c['dy']), tgt.to(_tap_major(c['w']))
    y = ops.dwconv_fwd(xd, wd, None, B, H, W, C, dil, None)
    _check_bound('fwd', y, c['y'], c['ya'], r)
    for ipg in ipgs:
        G = B // ipg
        ws = _new_ws(tgt, G, C)
        y2 = ops.dwconv_fwd(xd, wd, None, B, H, W, C, dil, None, colstats=(ws, ipg))
        assert torch.equal(y2, y)
        st = _read_stats(ws, G, C)
        yg, ag = c['y'].reshape(G, ipg * H * W, C), c['ya'].reshape(G, ipg * H * W, C)
        _check_bound(f'column sums ({ipg} per group)', st[:, 0], yg.sum(1), ag.sum(1), 0.0)
        _check_bound(f'column sums of squares ({ipg} per group)', st[:, 1], (yg * yg).sum(1), 2 * (ag * yg.abs()).sum(1), 0.0)
    dx = ops.dwconv_bwd_data(dyd, wd, B, H, W, C, dil)
    _check_bound('dx', dx, c['dx'], c['dxa'], r)
    acc = ops.dwconv_bwd_data(dyd, wd, B, H, W, C, dil, out=tgt.to(c['prev'].clone()), accumulate=True)
    _check_bound('dx accumulated', acc, c['dx'] + c['prev'].double(), c['dxa'] + c['prev'].double().abs(), r)
    dw, db = torch.zeros(C, 9, device=tgt.device), torch.zeros(C, device=tgt.device)
    ops.dwconv_bwd_weight(dyd, xd, dw, db, B, H, W, C, dil)
    _check_bound('dweight', dw, c['dw'], c['dwa'], 0.0)
    _check_bound('dbias', db, c['dy'].double().sum((0, 1, 2)), c['dy'].double().abs().sum((0, 1, 2)), 0.0)


# ====================================================================================================== 3. dilation with GELU
# dw_stencil_kernel MODE 0 with act == 2, MODE 1 (the backward prep) and dw_gelu_bwd_fused_kernel at dil >= 2, at exactly the tolerances
# test_kernels.test_dwconv applies to its dilation-1 GELU case (the device erf polynomial's error is in those figures).
GELU_TOL = {FP32: 3e-5, BF16: 1.6e-2}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('dil', [2, 6])
@pytest.mark.parametrize('shape', [(2, 13, 9, 24), (1, 23, 12, 68)])
def test_dilated_gelu(tgt, dt, dil, shape):
    B, H, W, C = shape
    tol = GELU_TOL[dt]
    torch.manual_seed(dil * 100 + H)
    x, dy, prev = torch.randn(B, H, W, C).to(dt), torch.randn(B, H, W, C).to(dt), torch.randn(B, H, W, C).to(dt)
    w, b = torch.randn(C, 1, 3, 3) * 0.3, torch.randn(C)
    _, y_ref, dx_ref, dw_ref, db_ref = _ref64(x, w, dy, dil, bias=b, gelu=True)
    xd, wd, bd, dyd = tgt.to(x), tgt.to(_tap_major(w)), tgt.to(b), tgt.to(dy)
    y = ops.dwconv_fwd(xd, wd, bd, B, H, W, C, dil, 'gelu')
    assert_close(y, y_ref, tol, name='dw fwd')
    dz = ops.dwconv_gelu_bwd_prep(xd, wd, bd, dyd, B, H, W, C, dil)
    dx = ops.dwconv_bwd_data(dz, wd, B, H, W, C, dil)
    assert_close(dx, dx_ref, tol * 2, name='dw dx')
    acc = ops.dwconv_bwd_data(dz, wd, B, H, W, C, dil, out=tgt.to(prev.clone()), accumulate=True)
    assert_close(acc, dx_ref + prev.double(), tol * 3, name='dw dx accumulate')
    dw, db = torch.zeros(C, 9, device=tgt.device), torch.zeros(C, device=tgt.device)
    ops.dwconv_bwd_weight(dz, xd, dw, db, B, H, W, C, dil)
    assert_close(dw, dw_ref, tol, name='dw dweight')
    assert_close(db, db_ref, tol, name='dw dbias')
    dw2, db2 = torch.zeros(C, 9, device=tgt.device), torch.zeros(C, device=tgt.device)
    dz2 = ops.dwconv_gelu_bwd_fused(xd, wd, bd, dyd, dw2, db2, B, H, W, C, dil)
    assert_close(dz2, dz, 1e-6 if dt == FP32 else 4e-3, name='fused dz')
    assert_close(dw2, dw_ref, tol, name='fused dweight')
    assert_close(db2, db_ref, tol, name='fused dbias')


# ====================================================================================================== 4. refusals at the ABI
OK, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -4
SENTINEL = 7.0


class _Abi:
    """every dwconv entry point on one set of buffers (sized for 1 x 4 x 4 x 8), outputs pre-filled with a sentinel"""
    NAMES = ('fwd', 'fwd_stats', 'gelu_bwd_prep', 'bwd_data', 'bwd_weight', 'gelu_bwd_fused')

    def __init__(self, tgt, dt):
        self.dt = dt
        mk = lambda n, d, v: torch.full((n,), v, dtype=d, device=tgt.device)
        self.x, self.da = mk(128, dt, 1.0), mk(128, dt, 1.0)
        self.w, self.bias = mk(72, FP32, 1.0), mk(8, FP32, 1.0)
        self.out = mk(128, dt, SENTINEL)
        self.dw, self.db, self.ws = mk(72, FP32, SENTINEL), mk(8, FP32, SENTINEL), mk(2 * 66 * 8, FP32, SENTINEL)

    def call(self, name, B, H, W, C, dil, ws='own', ipg=1):
        lib, p, i = L.lib(), L.ptr, L.c_i32
        tag, s = L.dtype_tag(self.x), L.stream_of(self.x)
        dims = (i(B), i(H), i(W), i(C), i(dil))
        x, w, b, da, out, dw, db = map(p, (self.x, self.w, self.bias, self.da, self.out, self.dw, self.db))
        if name == 'fwd':
            return lib.cmda_dwconv3x3_fwd(x, w, b, out, *dims, i(0), tag, s)
        if name == 'fwd_stats':
            return lib.cmda_dwconv3x3_fwd_stats(x, w, b, out, *dims, p(self.ws) if ws == 'own' else None, i(ipg), tag, s)
        if name == 'gelu_bwd_prep':
            return lib.cmda_dwconv3x3_gelu_bwd_prep(x, w, b, da, out, *dims, tag, s)
        if name == 'bwd_data':
            return lib.cmda_dwconv3x3_bwd_data(da, w, out, *dims, i(0), tag, s)
        if name == 'bwd_weight':
            return lib.cmda_dwconv3x3_bwd_weight(da, x, dw, db, *dims, tag, s)
        if name == 'gelu_bwd_fused':
            return lib.cmda_dwconv3x3_gelu_bwd_fused(x, w, b, da, out, dw, db, *dims, tag, s)
        raise AssertionError(name)

    def untouched(self):
        return all(bool((t.float() == SENTINEL).all().item()) for t in (self.out, self.dw, self.db, self.ws))


@pytest.mark.parametrize('dt', DTYPES)
def test_abi_refusals(tgt, dt):
    a = _Abi(tgt, dt)
    # the statistics exist on the dilated walk only, for whole groups, into a workspace
    assert a.call('fwd_stats', 1, 4, 4, 8, 1) == ERR_UNSUPPORTED
    assert a.call('fwd_stats', 1, 4, 4, 8, 0) == ERR_UNSUPPORTED   # (dil < 2 is refused before the shape is looked at)
    assert a.call('fwd_stats', 1, 4, 4, 8, 2, ws=None) == ERR_UNSUPPORTED
    assert a.call('fwd_stats', 3, 1, 4, 8, 2, ipg=2) == ERR_UNSUPPORTED
    assert a.call('fwd_stats', 2, 2, 4, 8, 2, ipg=0) == ERR_UNSUPPORTED
    for name in a.NAMES:
        assert a.call(name, 1, 4, 4, 6, 2) == ERR_SHAPE, f'{name}: C % 4 != 0'
        if name != 'fwd_stats':
            assert a.call(name, 1, 4, 4, 8, 0) == ERR_SHAPE, f'{name}: dil = 0'
            assert a.call(name, 1, 4, 4, 8, -1) == ERR_SHAPE, f'{name}: dil < 0'
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert a.untouched(), 'a refused call wrote to an output'


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('zero', ['B', 'H', 'W', 'C'])
def test_abi_zero_sized_problem(tgt, dt, zero):
    a = _Abi(tgt, dt)
    dims = dict(B=1, H=4, W=4, C=8)
    dims[zero] = 0
    for name in a.NAMES:
        assert a.call(name, dims['B'], dims['H'], dims['W'], dims['C'], 2) == OK, name
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert a.untouched(), 'a zero-sized problem wrote to an output'
