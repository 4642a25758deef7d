"""The GEMM family (cmda_amd/csrc/gemm*.hip, gemm_kernels.h) against float64 torch, bit for bit.

Operands are small integers (split-bf16 low halves: integers plus j / 1024), epilogue scalars powers of two.  Every product and every
partial sum -- in ANY order: MFMA accumulation, split-K atomics, LDS staging, tile walks -- is then exactly representable in fp32, so
the fp32 result IS the float64 result and a bf16 store is one round-to-nearest-even of it.  The comparison is torch.equal; `exact_bound`
asserts the condition the argument rests on for every case.  GELU / tanh epilogues are not exact and stay in test_gemm.py.

Every launch is planned first (cmda_debug_gemm_plan) and must agree with its plan: it runs exactly when the plan is no refusal.  The last
test of the file walks the same cases again with the launches left out, collects their plans, and asserts which kernel families, tiles
and LDS-DMA stage counts they reach, and caps the share of refused combinations -- in whatever order or process the cases themselves ran.

This file sets ops.GEMM_TILE_HINT itself (test_gemm.py's forced-tile children do not run it)."""
import collections
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from cmda_amd import _lib as L
from cmda_amd import deferred, ops
from cmda_amd._lib import CmdaError
from test_gemm import CONVS

BF, F32 = torch.bfloat16, torch.float32
MODES = [pytest.param(F32, 0, id='fp32'), pytest.param(BF, 1, id='bf16'), pytest.param(F32, 2, id='x3')]
# 1..4: forced tile; 4 | 512: the general kernel's 256x256 tile; 4 | 1024: the ping-pong kernel; 8192: no lean kernel; 65536: the lean split kernel
HINTS = (0, 1, 2, 3, 4, 516, 1028, 8192, 65536)
FEW = (0, 3, 8192, 65536)     # the largest shapes: the library's choice, the small-tile (lean) kernels, the general ones
# Hints that cannot change a mode's launch are left out (plan_gemm): the 256x256 tile exists on the bf16 LDS-DMA path only -- in the fp32
# modes 4, 516 and 1028 plan exactly what 1 plans --, bit 13 switches between the bf16 and the split-bf16 lean kernels and their general
# counterparts, bit 16 concerns the split-bf16 mode alone.  {mode: {hint left out: the hint that plans the same launch}}; the plain cases
# assert the equality of the plans.
SAME_AS_ANOTHER = {0: {4: 1, 516: 1, 1028: 1, 8192: 0, 65536: 0}, 1: {65536: 0}, 2: {4: 1, 516: 1, 1028: 1}}
FAMILY = ('NONE', 'PINGPONG', 'WGRAD', 'GLDS', 'LEAN', 'REG', 'X3REG', 'X3LEAN')
TILE = ('T128', 'T128x64', 'T64', 'T256')

# the coverage test's walk over the cases (PLAN_ONLY: nothing is launched or compared, the plans are counted)
PLAN_ONLY = [False]
PLANS = collections.Counter()     # (family, tile, stages, waves) -> launches
TALLY = collections.Counter()     # 'ran' / 'refused' launches
REFUSED = collections.Counter()   # (what, mode) -> refused launches


def hints_of(tag, hints=HINTS):
    return tuple(h for h in hints if h not in SAME_AS_ANOTHER[tag])


@pytest.fixture(autouse=True)
def _switches_restored():
    saved = (ops.GEMM_TILE_HINT, ops.X3_BIG_FLOPS, ops.X3_BIG_INTENSITY, ops.GEMM_DEFER)
    try:
        yield
    finally:
        ops.GEMM_TILE_HINT, ops.X3_BIG_FLOPS, ops.X3_BIG_INTENSITY, ops.GEMM_DEFER = saved


# ---------------------------------------------------------------------------------------------------------------- helpers
def ints(shape, lo=-3, hi=3, dt=F32):
    """integer-valued tensor of the storage type (|values| <= 4 are exact in bf16)"""
    return torch.randint(lo, hi + 1, tuple(shape)).to(dt)


def low_halves(shape):
    """int + j / 1024, j in [-7, 7]: fp32 values whose bf16 split x = hi + lo has a non-zero low half, both halves on the 2^-10 grid"""
    return ints(shape) + torch.randint(-7, 8, tuple(shape)).float() / 1024


def exact_bound(absprod, *terms, grid=1.0):
    """the condition of the method (not a measurement): the largest magnitude any partial sum can reach stays below 2^24 grid steps,
    so every partial sum in every order is an fp32 number.  A case that trips this is re-ranged, never given a tolerance."""
    worst = absprod.double().abs().max().item() + sum(t.double().abs().max().item() for t in terms if t is not None)
    assert worst < 2.0 ** 24 * grid, f'case out of the exact range: {worst} >= 2^24 * {grid}'


def well_above_256(acc):
    """precision cases: a bf16 rounding in the wrong place must not be able to hide (bf16 spacing above 256 is >= 2)"""
    assert (acc.abs() > 256).double().mean().item() >= 0.9


def expect(out, ref64, what):
    if PLAN_ONLY[0]:
        return
    assert torch.equal(ref64.float().double(), ref64), f'{what}: the float64 reference is not an fp32 number (case out of range)'
    want = ref64.float().to(out.dtype)
    got = out.detach().cpu()
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}'
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    d = (got.double() - want.double()).abs()[bad]
    first = tuple(bad.nonzero()[0].tolist())
    pytest.fail(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |diff| {d.max().item()}, first at {first}: '
                f'got {got[first].item()}, want {want[first].item()}')


def plan_of(A, B, out, M, N, K, whole=False, **kw):
    """(return code, family, tile, stages, waves, splits) the library plans for this launch -- host only, nothing runs"""
    p = ops.gemm(A, B, out, M, N, K, hold=True, **kw)[0]
    o = (ctypes.c_int32 * 7)()
    assert L.lib().cmda_debug_gemm_plan(ctypes.byref(p), o) == 0
    return tuple(o) if whole else tuple(o)[:6]


def plan_name(pl):
    return f'{FAMILY[pl[1]]}/{TILE[pl[2]]}/{pl[3]} stages/{pl[4]} waves/{pl[5]} splits' if pl and pl[0] == 0 else str(pl)


def launch(tgt, A, B, out, M, N, K, big=False, what='', **kw):
    """plan, then launch.  Returns the plan's name, or None where the library refuses the combination; a launch and its plan must agree.
    big: the three-launch path of ops._gemm_x3_big (three bf16 launches behind one call: no single plan to compare with)"""
    pl = None if big else plan_of(A, B, out, M, N, K, **kw)
    if PLAN_ONLY[0]:
        if pl is not None and pl[0] != 0:
            TALLY['refused'] += 1
            REFUSED[(what.split(':')[-1].strip(), kw.get('dtype'))] += 1
            return None
        TALLY['ran'] += 1
        if pl is not None:
            PLANS[pl[1:5]] += 1
        return plan_name(pl) if pl else 'three launches'
    try:
        ops.gemm(A, B, out, M, N, K, **kw)
    except CmdaError as e:
        if 'unsupported' not in str(e):
            raise
        assert pl is None or pl[0] != 0, f'{what} [hint {ops.GEMM_TILE_HINT}]: planned as {plan_name(pl)}, yet the launch was refused'
        return None
    assert pl is None or pl[0] == 0, f'{what} [hint {ops.GEMM_TILE_HINT}]: planned as a refusal {pl}, yet it ran'
    return plan_name(pl) if pl else 'three launches'


def go(tgt, what, ref64, out, A, B, M, N, K, **kw):
    name = launch(tgt, A, B, out, M, N, K, what=what, **kw)
    if name is not None:
        expect(out, ref64, f'{what} [hint {ops.GEMM_TILE_HINT}: {name}]')
    return name is not None


def khwc(w):   # [Co,Ci,KH,KW] -> the implicit GEMM's [Co, (kh,kw,ci)]
    return w.permute(0, 2, 3, 1).contiguous().view(w.shape[0], -1)


def dgrad_w(w):   # [Co,Ci,KH,KW] -> [Ci, (kh,kw,co)] with the taps flipped (runtime.wconv(..., 'dgrad'))
    return w.flip(2, 3).permute(1, 2, 3, 0).contiguous().view(w.shape[1], -1)


def nchw(t):
    return t.double().permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- plain operands
PLAIN = [(70, 50, 40), (130, 19, 147), (33, 200, 8), (129, 65, 1), (300, 260, 96),
         (257, 96, 768), (129, 64, 1024), (256, 128, 64)]   # >= 12 k-tiles / whole 64-deep k-tiles: the lean and 4-stage configurations


def _plain_problem(M, N, K, dt):
    torch.manual_seed(M * 7 + N)
    lo, hi = (-1, 4) if K >= 256 else (-3, 3)   # non-centred: accumulators of a deep contraction sit far above 2^8
    a, b = ints((M, K), lo, hi, dt), ints((N, K), lo, hi, dt)
    bias, res, c0 = ints((N,)), ints((M, N), dt=dt), ints((M, N), dt=dt)
    acc = a.double() @ b.double().t()
    exact_bound(a.double().abs() @ b.double().abs().t(), bias, res, c0, grid=0.25)   # (alpha = 0.25, beta = 0.5 below)
    if K >= 256:
        well_above_256(acc)
    return a, b, bias, res, c0, acc


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('M,N,K', PLAIN)
def test_exact_plain_layouts(tgt, dt, tag, M, N, K):
    """NT, NT + bias + relu + residual, NN, TN with split-K atomics, K-strided A with beta = 1, alpha = 0.25 -- under every hint"""
    a, b, bias, res, c0, acc = _plain_problem(M, N, K, dt)
    ad, bd, biasd, resd = map(tgt.to, (a, b, bias, res))
    atd, btd = tgt.to(a.t().contiguous()), tgt.to(b.t().contiguous())
    A, B, At, Bt = ops.plain_view(ad, M, K), ops.plain_view(bd, N, K), ops.plain_view(atd, K, M), ops.plain_view(btd, K, N)
    new = lambda d=dt: torch.empty(M, N, dtype=d, device=tgt.device)
    for left_out, same in SAME_AS_ANOTHER[tag].items():   # the hints this mode's cases leave out plan what another hint plans
        for views, kw in (((A, B), dict(dtype=tag, bias=biasd, res=resd)),
                          ((At, Bt), dict(a_kstrided=True, b_kstrided=True, dtype=tag, atomic=True, splits=0))):
            plans = []
            for hint in (left_out, same):
                ops.GEMM_TILE_HINT = hint
                plans.append(plan_of(*views, torch.empty(M, N, device=tgt.device), M, N, K, whole=True, **kw))
            assert plans[0] == plans[1], f'mode {tag}: hint {left_out} plans {plans[0]}, hint {same} plans {plans[1]}'
    for hint in hints_of(tag, HINTS if M * N * K < 2e6 else FEW):
        ops.GEMM_TILE_HINT = hint
        go(tgt, 'NT', acc, new(), A, B, M, N, K, dtype=tag)
        go(tgt, 'NT + bias + relu + res', F.relu(acc + bias) + res.double(), new(), A, B, M, N, K, dtype=tag, bias=biasd, act='relu', res=resd)
        go(tgt, 'NN', acc, new(), A, Bt, M, N, K, b_kstrided=True, dtype=tag)
        go(tgt, 'TN split-K atomic', acc, torch.zeros(M, N, device=tgt.device), At, Bt, M, N, K, a_kstrided=True, b_kstrided=True,
           dtype=tag, atomic=True, splits=3)
        go(tgt, 'A k-strided, beta = 1', acc + c0.double(), tgt.to(c0.clone()), At, B, M, N, K, a_kstrided=True, dtype=tag, beta=1.0)
        go(tgt, 'NT alpha = 0.25', 0.25 * acc, new(), A, B, M, N, K, dtype=tag, alpha=0.25)


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('M,N,K', PLAIN)
def test_exact_plain_epilogues_strides_alignment(tgt, dt, tag, M, N, K):
    """the epilogue terms one by one, output types, leading dimensions beyond the matrix, operands off the 16-byte grid"""
    a, b, bias, res, c0, acc = _plain_problem(M, N, K, dt)
    res32 = ints((M, N))
    rps = 32
    rs = torch.tensor([0.5, 2.0, 1.0, 0.25])[torch.randint(0, 4, ((M + rps - 1) // rps,))]
    ad, bd, biasd, resd, res32d, rsd = map(tgt.to, (a, b, bias, res, res32, rs))
    A, B = ops.plain_view(ad, M, K), ops.plain_view(bd, N, K)
    rs_rows = rs.double().repeat_interleave(rps)[:M, None]
    # operands inside wider buffers (ld > cols, aligned offset) and off the 16-byte grid (element offset 1 / 3: vec_ok = 0)
    lda, ldb = (K + 7) // 8 * 8 + 16, (K + 7) // 8 * 8 + 8
    wide_a, wide_b = ints((M, lda), dt=dt), ints((N, ldb), dt=dt)
    wide_a[:, 8:8 + K], wide_b[:, 8:8 + K] = a, b
    odd_a, odd_b = torch.cat([ints((1,), dt=dt), a.flatten()]), torch.cat([ints((3,), dt=dt), b.flatten()])
    wad, wbd, oad, obd = map(tgt.to, (wide_a, wide_b, odd_a, odd_b))
    Aw, Bw = ops.plain_view(wad, M, K, ld=lda, offset=8), ops.plain_view(wbd, N, K, ld=ldb, offset=8)
    Ao, Bo = ops.plain_view(oad, M, K, offset=1), ops.plain_view(obd, N, K, offset=3)
    assert Aw.vec_ok and Bw.vec_ok and not Ao.vec_ok and not Bo.vec_ok
    ldc = N + 12
    frame = ints((M + 1, ldc), dt=dt)    # the output inside a wider buffer: what lies around it must come back untouched
    new = lambda d=dt: torch.empty(M, N, dtype=d, device=tgt.device)

    def framed(ref, off):
        want = frame.double().flatten().clone()
        idx = off + torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]
        want[idx.flatten()] = ref.flatten()
        return want.view(M + 1, ldc)
    for hint in hints_of(tag, FEW if M * N * K < 4e6 else (0, 8192)):
        ops.GEMM_TILE_HINT = hint
        go(tgt, 'bias', acc + bias, new(), A, B, M, N, K, dtype=tag, bias=biasd)
        go(tgt, 'bias + relu', F.relu(acc + bias), new(), A, B, M, N, K, dtype=tag, bias=biasd, act='relu')
        go(tgt, 'rowscale', F.relu(acc + bias) * rs_rows + res.double(), new(), A, B, M, N, K, dtype=tag, bias=biasd, act='relu',
           res=resd, rowscale=rsd, rows_per_scale=rps)
        go(tgt, 'beta = 0.5', 0.25 * acc + bias + 0.5 * c0.double(), tgt.to(c0.clone()), A, B, M, N, K, dtype=tag, alpha=0.25,
           bias=biasd, beta=0.5)
        if tag == 1:   # bf16 operands: fp32 output, and the fp32 residual stream next to bf16 storage
            go(tgt, 'fp32 output', acc + bias, new(F32), A, B, M, N, K, dtype=tag, bias=biasd)
            go(tgt, 'fp32 residual', F.relu(acc + bias) + res32.double(), new(), A, B, M, N, K, dtype=tag, bias=biasd, act='relu', res=res32d)
            go(tgt, 'fp32 residual, fp32 output', acc + res32.double(), new(F32), A, B, M, N, K, dtype=tag, res=res32d)
        go(tgt, 'ld > cols', acc + bias, new(), Aw, Bw, M, N, K, dtype=tag, bias=biasd)
        go(tgt, 'ldc > N, c_offset', framed(F.relu(acc + bias), 8), tgt.to(frame.clone()), A, B, M, N, K, dtype=tag, bias=biasd,
           act='relu', ldc=ldc, c_offset=8)
        go(tgt, 'unaligned operands', acc + bias, new(), Ao, Bo, M, N, K, dtype=tag, bias=biasd)
        go(tgt, 'unaligned output', framed(acc + res.double(), 1), tgt.to(frame.clone()), Ao, B, M, N, K, dtype=tag, res=resd, ldc=ldc,
           c_offset=1)


# (96, 72, 200) / (130, 19, 147): K is no multiple of the 32- / 64-deep k-tile times the split count -- a split boundary inside a k-tile
@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('M,N,K', [(70, 50, 40), (130, 19, 147), (96, 72, 200), (257, 96, 768)])
def test_exact_split_k_atomics(tgt, dt, tag, M, N, K):
    torch.manual_seed(K)
    a, b, c0 = ints((M, K), dt=dt), ints((N, K), dt=dt), ints((M, N), -50, 50)
    acc = a.double() @ b.double().t()
    exact_bound(a.double().abs() @ b.double().abs().t(), c0)
    ad, bd, atd, btd = tgt.to(a), tgt.to(b), tgt.to(a.t().contiguous()), tgt.to(b.t().contiguous())
    A, B, At, Bt = ops.plain_view(ad, M, K), ops.plain_view(bd, N, K), ops.plain_view(atd, K, M), ops.plain_view(btd, K, N)
    for hint in hints_of(tag, HINTS if M * N * K < 5e5 else FEW):
        ops.GEMM_TILE_HINT = hint
        for splits in (0, 2, 3, 5):
            go(tgt, f'TN, {splits} splits, zeroed', acc, torch.zeros(M, N, device=tgt.device), At, Bt, M, N, K, a_kstrided=True,
               b_kstrided=True, dtype=tag, atomic=True, splits=splits)
            go(tgt, f'TN, {splits} splits, pre-filled', acc + c0.double(), tgt.to(c0.clone()), At, Bt, M, N, K, a_kstrided=True,
               b_kstrided=True, dtype=tag, atomic=True, splits=splits)
            if splits in (0, 3):
                go(tgt, f'NT, {splits} splits, pre-filled', acc + c0.double(), tgt.to(c0.clone()), A, B, M, N, K, dtype=tag, atomic=True,
                   splits=splits)


@pytest.mark.parametrize('dt,tag', MODES)
def test_exact_batched_heads(tgt, dt, tag):
    """batch / batch2 with strides (attention scores of hd = 64 heads): one launch per head, and one launch over (batch, head)"""
    torch.manual_seed(1)
    Bn, Nq, Nk, h, hd = 2, 40, 24, 2, 64
    C = h * hd
    q, kv = ints((Bn, Nq, C), dt=dt), ints((Bn, Nk, 2 * C), dt=dt)
    qd, kvd = tgt.to(q), tgt.to(kv)
    qr = q.double().view(Bn, Nq, h, hd).permute(0, 2, 1, 3)
    kr = kv.double()[..., :C].reshape(Bn, Nk, h, hd).permute(0, 2, 1, 3)
    ref = 0.25 * qr @ kr.transpose(-1, -2)
    exact_bound(qr.abs() @ kr.abs().transpose(-1, -2), grid=0.25)
    for hint in hints_of(tag):
        ops.GEMM_TILE_HINT = hint
        S = torch.empty(Bn, h, Nq, Nk, dtype=dt, device=tgt.device)
        ran = [launch(tgt, ops.plain_view(qd, Nq, hd, ld=C, batch_stride=Nq * C, offset=hh * hd),
                      ops.plain_view(kvd, Nk, hd, ld=2 * C, batch_stride=Nk * 2 * C, offset=hh * hd),
                      S, Nq, Nk, hd, what='one launch per head', batch=Bn, c_batch_stride=h * Nq * Nk, c_offset=hh * Nq * Nk, dtype=tag,
                      alpha=0.25) for hh in range(h)]
        if all(ran):
            expect(S, ref, f'one launch per head [hint {hint}: {ran[0]}]')
        go(tgt, 'one launch over (batch, head)', ref, torch.empty(Bn, h, Nq, Nk, dtype=dt, device=tgt.device),
           ops.plain_view(qd, Nq, hd, ld=C, batch_stride=Nq * C, batch2_stride=hd),
           ops.plain_view(kvd, Nk, hd, ld=2 * C, batch_stride=Nk * 2 * C, batch2_stride=hd), Nq, Nk, hd, batch=Bn, batch2=h,
           c_batch_stride=h * Nq * Nk, c_batch2_stride=Nq * Nk, dtype=tag, alpha=0.25)


# ---------------------------------------------------------------------------------------------------------------- implicit-GEMM views
def _conv_problem(Bc, H, W, Ci, Co, KH, st, pd, dl, dt):
    torch.manual_seed(H + Ci)
    x, w, bias = ints((Bc, H, W, Ci), dt=dt), ints((Co, Ci, KH, KH), dt=dt), ints((Co,))
    xr, wr = nchw(x).requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=st, padding=pd, dilation=dl)
    dy = ints((Bc,) + tuple(y.shape[2:]) + (Co,), dt=dt)
    y.backward(nchw(dy))
    exact_bound(F.conv2d(nchw(x).abs(), w.double().abs(), stride=st, padding=pd, dilation=dl), bias)
    return x, w, bias, dy, y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('Bc,H,W,Ci,Co,KH,st,pd,dl', CONVS)
def test_exact_conv_views(tgt, dt, tag, Bc, H, W, Ci, Co, KH, st, pd, dl):
    """im2col / patch views: forward with bias + relu, the weight gradient with split-K atomics and the fused bias gradient into pre-filled
    gradients, the data gradient of the stride-1 geometries"""
    x, w, bias, dy, yref, dxref, dwref = _conv_problem(Bc, H, W, Ci, Co, KH, st, pd, dl, dt)
    OH, OW = yref.shape[1:3]
    M, K = Bc * OH * OW, KH * KH * Ci
    dw0, db0 = ints((Co, K), -50, 50), ints((Co,), -50, 50)
    exact_bound(torch.tensor(9.0 * M), dw0, db0)   # (a gradient element: at most M products of magnitude <= 9, plus the pre-fill)
    xd, dyd, wg, biasd = tgt.to(x), tgt.to(dy), tgt.to(khwc(w)), tgt.to(bias)
    wd = tgt.to(dgrad_w(w))
    dwk = dwref.permute(0, 2, 3, 1).reshape(Co, K) + dw0.double()
    dbref = dy.double().sum((0, 1, 2)) + db0.double()
    for hint in hints_of(tag, HINTS if M * K * Co < 5e5 else (1,) + FEW):
        ops.GEMM_TILE_HINT = hint
        go(tgt, 'conv forward + bias + relu', F.relu(yref + bias), torch.empty(Bc, OH, OW, Co, dtype=dt, device=tgt.device),
           ops.conv_view(xd, Bc, H, W, Ci, KH, KH, st, pd, dl), ops.plain_view(wg, Co, K), M, Co, K, dtype=tag, bias=biasd, act='relu')
        dW, db = tgt.to(dw0.clone()), tgt.to(db0.clone())
        wgrad = dict(a_kstrided=True, b_kstrided=True, dtype=tag, atomic=True, splits=2)
        views = (ops.plain_view(dyd, M, Co), ops.conv_view(xd, Bc, H, W, Ci, KH, KH, st, pd, dl))
        if go(tgt, 'conv weight gradient (with the bias gradient)', dwk, dW, *views, Co, K, M, colsum=db, **wgrad):
            expect(db, dbref, f'fused bias gradient [hint {hint}]')
        else:   # the fused bias gradient is refused here (counted): the weight gradient alone
            assert torch.equal(dW.cpu(), dw0) and torch.equal(db.cpu(), db0), 'a refused launch wrote'
            go(tgt, 'conv weight gradient', dwk, dW, *views, Co, K, M, **wgrad)
        if st == 1:
            go(tgt, 'conv data gradient', dxref, torch.empty(Bc, H, W, Ci, dtype=dt, device=tgt.device),
               ops.conv_view(dyd, Bc, OH, OW, Co, KH, KH, 1, dl * (KH - 1) - pd, dl, OH=H, OW=W), ops.plain_view(wd, Ci, KH * KH * Co),
               Bc * H * W, Ci, KH * KH * Co, dtype=tag)


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('Bc,H,W,Ci,Co,k,pd', [(2, 9, 11, 8, 24, 7, 3), (1, 5, 70, 16, 8, 3, 1),
                                               (1, 4, 4, 64, 16, 7, 3)])   # H = pad + 1: the smallest extent reflection is defined on
def test_exact_reflect_padded_view(tgt, dt, tag, Bc, H, W, Ci, Co, k, pd):
    """conv_view(reflect=1): the generator's 7x7 / 3x3 layers (cyclegan.py), against F.pad(mode='reflect') + conv2d"""
    torch.manual_seed(H * W)
    x, w, bias = ints((Bc, H, W, Ci), dt=dt), ints((Co, Ci, k, k), dt=dt), ints((Co,))
    xp = F.pad(nchw(x), (pd, pd, pd, pd), mode='reflect')
    yref = F.conv2d(xp, w.double()).permute(0, 2, 3, 1)
    exact_bound(F.conv2d(xp.abs(), w.double().abs()), bias)
    xd, wg, biasd = tgt.to(x), tgt.to(khwc(w)), tgt.to(bias)
    M, K = Bc * H * W, k * k * Ci
    for hint in hints_of(tag, HINTS if K < 3000 else (1,) + FEW):
        ops.GEMM_TILE_HINT = hint
        for odt in ({dt, F32} if hint in (0, 8192) else {dt}):   # (the generator keeps fp32 outputs in both modes)
            go(tgt, f'reflect-padded conv + bias + relu -> {odt}', F.relu(yref + bias), torch.empty(Bc, H, W, Co, dtype=odt, device=tgt.device),
               ops.conv_view(xd, Bc, H, W, Ci, k, k, 1, pd, 1, reflect=1), ops.plain_view(wg, Co, K), M, Co, K, dtype=tag, bias=biasd,
               act='relu')


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('Bc,H,W,Ci,Co,k,st,pd', [(2, 12, 12, 16, 8, 3, 2, 1), (1, 16, 16, 8, 16, 7, 4, 3), (1, 11, 13, 8, 8, 3, 2, 1),
                                                  (1, 9, 9, 8, 8, 4, 2, 1)])
def test_exact_input_dilated_view_strided_dgrad(tgt, dt, tag, Bc, H, W, Ci, Co, k, st, pd):
    """conv_view(in_dil=stride): the data gradient of a strided convolution (nn.conv_bwd), against autograd; beta = 0 and 1"""
    x, w, bias, dy, yref, dxref, dwref = _conv_problem(Bc, H, W, Ci, Co, k, st, pd, 1, dt)
    OH, OW = yref.shape[1:3]
    dx0 = ints((Bc, H, W, Ci), dt=dt)
    exact_bound(F.conv_transpose2d(nchw(dy).abs(), w.double().abs(), stride=st, padding=pd), dx0)
    dyd, wd = tgt.to(dy), tgt.to(dgrad_w(w))
    for hint in hints_of(tag):
        ops.GEMM_TILE_HINT = hint
        for beta in (0.0, 1.0):
            go(tgt, f'strided data gradient, beta = {beta}', dxref + beta * dx0.double(), tgt.to(dx0.clone()),
               ops.conv_view(dyd, Bc, OH, OW, Co, k, k, 1, k - 1 - pd, 1, OH=H, OW=W, in_dil=st), ops.plain_view(wd, Ci, k * k * Co),
               Bc * H * W, Ci, k * k * Co, dtype=tag, beta=beta)


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('Bc,H,W,Ci,Co,k,pd,opad', [(2, 6, 5, 16, 8, 3, 1, 1), (1, 9, 8, 8, 24, 4, 1, 0)])
def test_exact_transposed_convolution(tgt, dt, tag, Bc, H, W, Ci, Co, k, pd, opad):
    """the form cyclegan.py launches for ConvTranspose2d(stride 2): in_dil = 2, pad = KH - 2, fp32 output, against conv_transpose2d"""
    torch.manual_seed(k)
    x, w, bias = ints((Bc, H, W, Ci), dt=dt), ints((Ci, Co, k, k), dt=dt), ints((Co,))   # (ConvTranspose2d weights: [Ci, Co, KH, KW])
    yref = F.conv_transpose2d(nchw(x), w.double(), stride=2, padding=pd, output_padding=opad).permute(0, 2, 3, 1)
    assert tuple(yref.shape[1:3]) == (2 * H, 2 * W) and k - 1 - pd == k - 2
    exact_bound(F.conv_transpose2d(nchw(x).abs(), w.double().abs(), stride=2, padding=pd, output_padding=opad), bias)
    xd, wd, biasd = tgt.to(x), tgt.to(dgrad_w(w)), tgt.to(bias)
    for hint in hints_of(tag):
        ops.GEMM_TILE_HINT = hint
        go(tgt, 'transposed convolution', yref + bias, torch.empty(Bc, 2 * H, 2 * W, Co, device=tgt.device),
           ops.conv_view(xd, Bc, H, W, Ci, k, k, 1, k - 2, 1, OH=2 * H, OW=2 * W, in_dil=2), ops.plain_view(wd, Co, k * k * Ci),
           Bc * 4 * H * W, Co, k * k * Ci, dtype=tag, bias=biasd)


@pytest.mark.parametrize('dt,tag', MODES)
@pytest.mark.parametrize('Bc,H,W,Ci,Co,KH,st,pd,dl', [CONVS[0], CONVS[2], CONVS[3], CONVS[6], CONVS[8], CONVS[14]])
def test_exact_permuted_weight_gradient_store(tgt, dt, tag, Bc, H, W, Ci, Co, KH, st, pd, dl):
    """c_perm = (Ci, KH * KW): the weight gradient accumulated straight into the parameter's [Co, Ci, KH, KW] layout (nn.conv_bwd outside a
    backward scope), launched directly into a pre-filled gradient, the split count left to the library; against autograd"""
    x, w, bias, dy, yref, dxref, dwref = _conv_problem(Bc, H, W, Ci, Co, KH, st, pd, dl, dt)
    OH, OW = yref.shape[1:3]
    M, K = Bc * OH * OW, KH * KH * Ci
    g0, db0 = ints((Co, Ci, KH, KH), -50, 50), ints((Co,), -50, 50)
    exact_bound(torch.tensor(9.0 * M), g0, db0)
    xd, dyd = tgt.to(x), tgt.to(dy)
    for hint in hints_of(tag):
        ops.GEMM_TILE_HINT = hint
        views = (ops.plain_view(dyd, M, Co), ops.conv_view(xd, Bc, H, W, Ci, KH, KH, st, pd, dl))
        kw = dict(a_kstrided=True, b_kstrided=True, dtype=tag, atomic=True, splits=0, c_perm=(Ci, KH * KH))
        g, db = tgt.to(g0.clone()), tgt.to(db0.clone())
        if go(tgt, 'permuted weight gradient (with the bias gradient)', dwref + g0.double(), g, *views, Co, K, M, colsum=db, **kw):
            expect(db, dy.double().sum((0, 1, 2)) + db0.double(), f'fused bias gradient [hint {hint}]')
        else:
            assert torch.equal(g.cpu(), g0), 'a refused launch wrote'
            go(tgt, 'permuted weight gradient', dwref + g0.double(), g, *views, Co, K, M, **kw)


# ---------------------------------------------------------------------------------------------------------------- stores
@pytest.mark.parametrize('dt,tag,B,OH,OW,Co,Ci,k', [(F32, 0, 2, 3, 5, 24, 8, 2), (BF, 1, 2, 3, 5, 64, 32, 2), (BF, 1, 3, 4, 8, 128, 64, 4),
                                                    (BF, 1, 1, 9, 7, 192, 8, 2), (F32, 2, 2, 3, 5, 64, 32, 2), (F32, 2, 3, 4, 8, 128, 64, 4),
                                                    (F32, 2, 1, 9, 7, 96, 8, 2)])
def test_exact_unpatchify_store(tgt, dt, tag, B, OH, OW, Co, Ci, k):
    """c_patch: the data gradient of a kernel == stride convolution stored straight in NHWC, against conv_transpose2d; beta 0 and 1"""
    torch.manual_seed(5)
    dy, w, prev = ints((B, Co, OH, OW), dt=dt), ints((Co, Ci, k, k), dt=dt), ints((B * OH * k * OW * k, Ci), dt=dt)
    want = F.conv_transpose2d(dy.double(), w.double(), stride=k).permute(0, 2, 3, 1).reshape(-1, Ci)
    exact_bound(F.conv_transpose2d(dy.double().abs(), w.double().abs(), stride=k), prev)
    dy_rows = tgt.to(dy.permute(0, 2, 3, 1).reshape(-1, Co).contiguous())
    wg = tgt.to(khwc(w))
    M, K = B * OH * OW, k * k * Ci
    for hint in hints_of(tag):
        ops.GEMM_TILE_HINT = hint
        for beta in (0.0, 1.0):
            go(tgt, f'unpatchify, beta = {beta}', want + beta * prev.double(), tgt.to(prev.clone()), ops.plain_view(dy_rows, M, Co),
               ops.plain_view(wg, Co, K), M, K, Co, b_kstrided=True, dtype=tag, beta=beta, c_patch=(OW, k, k * Ci))


@pytest.mark.parametrize('dt,tag', MODES)
def test_exact_fused_column_statistics(tgt, dt, tag):
    """colstats: per-group column sums and sums of squares of the output, accumulated by the epilogue, equal float64 exactly; then
    bn_train_fwd(stats_ws=...) hands the workspace back all zero"""
    torch.manual_seed(11)
    groups, rpg, N, K = 2, 256, 72, 32
    M = groups * rpg
    a, b, bias, res = ints((M, K), -1, 1, dt), ints((N, K), -1, 1, dt), ints((N,), -2, 2), ints((M, N), -1, 1, dt)
    ad, bd, biasd, resd = map(tgt.to, (a, b, bias, res))
    wsn = int(L.lib().cmda_bn_ws_floats(N))
    for use_res in (True, False):   # (the ping-pong kernel takes no residual)
        ref = a.double() @ b.double().t() + bias + (res.double() if use_res else 0.0)
        exact_bound(a.double().abs() @ b.double().abs().t(), bias, res)
        assert rpg * (ref * ref).max().item() < 2.0 ** 24
        assert ref.abs().max().item() <= 256   # integers bf16 holds exactly: the sums of the stored and of the unrounded values coincide
        rg = ref.view(groups, rpg, N)
        for hint in hints_of(tag):
            ops.GEMM_TILE_HINT = hint
            for odt in {dt, F32}:
                ws = torch.zeros(groups * wsn, device=tgt.device)
                out = torch.empty(M, N, dtype=odt, device=tgt.device)
                if not go(tgt, f'output next to the statistics -> {odt}', ref, out, ops.plain_view(ad, M, K), ops.plain_view(bd, N, K),
                          M, N, K, dtype=tag, bias=biasd, res=resd if use_res else None, colstats=(ws, rpg)):
                    continue
                slots = ws.cpu().view(groups, 33, 2, N)
                st = slots[:, :32].double().sum(1)   # [group][sum | sum of squares][channel]
                expect(st[:, 0], rg.sum(1), f'column sums [hint {hint}]')
                expect(st[:, 1], (rg * rg).sum(1), f'column sums of squares [hint {hint}]')
                assert slots[:, 32].abs().max().item() == 0.0
                if PLAN_ONLY[0]:
                    continue
                g, be = tgt.to(torch.rand(N) + 0.5), tgt.to(torch.randn(N))
                rm, rv = torch.zeros(N, device=tgt.device), torch.ones(N, device=tgt.device)
                ops.GEMM_TILE_HINT = 0
                ops.bn_train_fwd(out, g, be, torch.empty_like(out), rm, rv, rpg, N, 1e-5, 0.1, True, groups=groups, stats_ws=ws)
                assert ws.abs().max().item() == 0.0, 'the workspace comes back zeroed'
                ops.GEMM_TILE_HINT = hint


# ---------------------------------------------------------------------------------------------------------------- split-bf16 low halves
def _low_half_launches(tgt, M, N, K, side, big=False):
    """integer operands have zero low halves: here ONE operand is int + j / 1024 (the hi * lo and lo * hi terms carry the result, the
    dropped lo * lo term is exactly zero) and everything lies on the 2^-10 grid"""
    a = low_halves((M, K)) if side == 'A' else ints((M, K))
    b = low_halves((N, K)) if side == 'B' else ints((N, K))
    bias, res, c0, cs0 = ints((N,)), low_halves((M, N)), ints((M, N), -50, 50), ints((M,), -50, 50)
    acc = a.double() @ b.double().t()
    exact_bound(a.double().abs() @ b.double().abs().t(), bias, res, c0, grid=2.0 ** -12)   # (2^-10 operands, alpha = 0.25)
    exact_bound(a.double().abs().sum(1) + 50, grid=2.0 ** -10)
    assert (a.bfloat16().float() != a).any() or (b.bfloat16().float() != b).any()
    ad, bd, biasd, resd = map(tgt.to, (a, b, bias, res))
    atd, btd = tgt.to(a.t().contiguous()), tgt.to(b.t().contiguous())
    A, B, At, Bt = ops.plain_view(ad, M, K), ops.plain_view(bd, N, K), ops.plain_view(atd, K, M), ops.plain_view(btd, K, N)
    what = f'low half in {side}'
    go(tgt, f'{what}: NT + bias + res + beta', acc + bias + res.double() + 0.5 * c0.double(), tgt.to(c0.clone()), A, B, M, N, K, big=big,
       dtype=2, bias=biasd, res=resd, beta=0.5)
    go(tgt, f'{what}: NN', acc, torch.empty(M, N, device=tgt.device), A, Bt, M, N, K, big=big, dtype=2, b_kstrided=True)
    act = None if big else 'relu'   # (an activation keeps a problem off the three-launch path)
    go(tgt, f'{what}: NT alpha = 0.25 + bias + {act}', (acc * 0.25 + bias) if big else F.relu(0.25 * acc + bias),
       torch.empty(M, N, device=tgt.device), A, B, M, N, K, big=big, dtype=2, alpha=0.25, bias=biasd, act=act)
    dW, cs = tgt.to(c0.clone()), tgt.to(cs0.clone())
    kw = dict(a_kstrided=True, b_kstrided=True, dtype=2, atomic=True, splits=0, big=big)
    if go(tgt, f'{what}: weight-gradient form with the bias gradient', acc + c0.double(), dW, At, Bt, M, N, K, colsum=cs, **kw):
        expect(cs, a.double().sum(1) + cs0.double(), f'{what}: fused bias gradient [hint {ops.GEMM_TILE_HINT}]')
    else:
        assert torch.equal(dW.cpu(), c0), 'a refused launch wrote'
        go(tgt, f'{what}: weight-gradient form', acc + c0.double(), dW, At, Bt, M, N, K, **kw)


# K = 64 / 128 / 1024: token counts that are whole 32-deep k-tiles -- the lean split kernel's weight-gradient form with the bias gradient
@pytest.mark.parametrize('side', ['A', 'B'])
@pytest.mark.parametrize('M,N,K', [(70, 52, 40), (130, 20, 147), (256, 128, 64), (200, 72, 128), (129, 64, 1024)])
def test_exact_split_bf16_low_halves(tgt, M, N, K, side):
    torch.manual_seed(M + K)
    for hint in (0, 8192, 65536):
        ops.GEMM_TILE_HINT = hint
        _low_half_launches(tgt, M, N, K, side)


@pytest.mark.parametrize('side', ['A', 'B'])
@pytest.mark.parametrize('M,N,K', [(200, 72, 128), (96, 40, 200)])
def test_exact_split_bf16_low_halves_three_launch_path(tgt, M, N, K, side):
    """ops._gemm_x3_big, forced by lowering its thresholds: the operands split once into bf16 halves, three launches of the bf16 kernels"""
    torch.manual_seed(M + K)
    ops.X3_BIG_FLOPS, ops.X3_BIG_INTENSITY = 1e3, 0.0
    _low_half_launches(tgt, M, N, K, side, big=True)
    # an im2col view on the same path
    x = low_halves((2, 12, 12, 16)) if side == 'A' else ints((2, 12, 12, 16))
    w = low_halves((24, 16, 3, 3)) if side == 'B' else ints((24, 16, 3, 3))
    exact_bound(F.conv2d(nchw(x).abs(), w.double().abs(), padding=1), grid=2.0 ** -10)
    xd, wg = tgt.to(x), tgt.to(khwc(w))
    go(tgt, f'low half in {side}: im2col view', F.conv2d(nchw(x), w.double(), padding=1).permute(0, 2, 3, 1),
       torch.empty(2, 12, 12, 24, device=tgt.device), ops.conv_view(xd, 2, 12, 12, 16, 3, 3, 1, 1, 1), ops.plain_view(wg, 24, 144),
       288, 24, 144, big=True, dtype=2)


# ---------------------------------------------------------------------------------------------------------------- deferred grouped
@pytest.mark.parametrize('dt,tag', MODES)
def test_exact_deferred_grouped_weight_gradients(tgt, dt, tag):
    """gemm(defer=True) inside a backward scope: the grouped launches (gemm_grouped.hip's tiles, gemm_wg.hip's 256x256 tile) of integer
    dy / x into pre-filled integer gradients.  grouped == one by one == float64, bias gradients included."""
    from cmda_amd import nn as K
    import cmda_amd.runtime as rt
    torch.manual_seed(5)
    rt.set_compute_dtype(dt)
    rt.set_gemm_x3(tag == 2)
    try:
        # (rows, out, in): a 64-wide and a ragged small problem, a 128-wide one, a 256x256-tile one, whole 32-deep k-tiles (the lean
        # split kernel's grouped form)
        shapes = [(520, 64, 64), (700, 72, 40), (3300, 128, 256), (3000, 320, 320), (4096, 320, 320), (96, 128, 128)]
        lins = [(ints((rows, n), dt=dt), ints((rows, k), dt=dt), torch.nn.Parameter(tgt.to(torch.randn(n, k))),
                 torch.nn.Parameter(tgt.to(torch.randn(n))), ints((n, k), -50, 50), ints((n,), -50, 50)) for rows, n, k in shapes]
        # a patch view, a 3x3 im2col, the OW = 64 patch view on the 256x256 tile's 32-deep kernel
        convs = [(2, 16, 16, 32, 24, 2, 2, 0), (1, 12, 20, 16, 16, 3, 1, 1), (1, 4, 128, 64, 256, 2, 2, 0)]
        cvs = []
        for Bc, H, W, Ci, Co, k, st, pd in convs:
            OH, OW = K.conv_out_size(H, W, k, st, pd)
            cvs.append((ints((Bc * OH * OW, Co), dt=dt), ints((Bc, H, W, Ci), dt=dt), torch.nn.Parameter(tgt.to(torch.randn(Co, Ci, k, k))),
                        torch.nn.Parameter(tgt.to(torch.randn(Co))), ints((Co, Ci, k, k), -50, 50), ints((Co,), -50, 50), (Bc, H, W, st, pd)))
        exact_bound(torch.tensor(9.0 * 4096 + 50))   # every gradient element: at most 4096 products of magnitude <= 9, plus the pre-fill

        def run(defer):
            ops.GEMM_DEFER = defer
            for e in lins + cvs:
                e[2].grad, e[3].grad = tgt.to(e[4].clone()), tgt.to(e[5].clone())
            with ops.backward_scope():
                for dy, x, w, b, _, _ in lins:
                    K.linear_bwd(tgt.to(dy), tgt.to(x), w, b, dy.shape[0], x.shape[1], need_dx=False)
                for dy, x, w, b, _, _, (Bc, H, W, st, pd) in cvs:
                    K.conv_bwd(tgt.to(dy), tgt.to(x.reshape(-1, x.shape[-1])), w, b, Bc, H, W, st, pd, need_dx=False)
                assert bool(deferred.GEMM.pending) == bool(defer)
            assert not deferred.GEMM.pending
            return [(e[2].grad.cpu().clone(), e[3].grad.cpu().clone()) for e in lins + cvs]
        single, grouped = run(False), run(True)
        want = []
        for dy, x, w, b, g0, b0 in lins:
            want.append((dy.double().t() @ x.double() + g0.double(), dy.double().sum(0) + b0.double()))
        for dy, x, w, b, g0, b0, (Bc, H, W, st, pd) in cvs:
            wr = torch.zeros(w.shape, dtype=torch.float64, requires_grad=True)
            y = F.conv2d(nchw(x), wr, None, st, pd)
            y.backward(dy.double().view(Bc, y.shape[2], y.shape[3], -1).permute(0, 3, 1, 2))
            want.append((wr.grad + g0.double(), dy.double().sum(0) + b0.double()))
        for i, ((sw, sb), (gw, gb), (ww, wb)) in enumerate(zip(single, grouped, want)):
            expect(sw, ww, f'problem {i}: weight gradient, launched alone')
            expect(sb, wb, f'problem {i}: bias gradient, launched alone')
            expect(gw, ww, f'problem {i}: weight gradient, grouped launch')
            expect(gb, wb, f'problem {i}: bias gradient, grouped launch')
    finally:
        ops.GEMM_DEFER = True
        rt.set_gemm_x3(False)
        rt.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------------------------- coverage
def _cases_of(fn):
    """the parameter sets of a parametrised test function, as keyword dictionaries"""
    sets = []
    for m in fn.pytestmark:
        if m.name == 'parametrize':
            names = [n.strip() for n in m.args[0].split(',')]
            rows = [v.values if hasattr(v, 'values') else (v if len(names) > 1 else (v,)) for v in m.args[1]]
            sets.append([dict(zip(names, r)) for r in rows])
    for combo in itertools.product(*sets):
        yield {k: v for d in combo for k, v in d.items()}


def test_exact_cases_reach_every_family_tile_and_stage_count(tgt):
    """LAST in the file.  Walks every cmda_gemm case above once more on this target with the launches left out (every case asserts, where it
    runs, that a launch runs exactly when its plan is no refusal -- so the plans ARE what ran) and checks what they reach.
    kGemmWgrad: left to itself cmda_gemm plans it only at sizes far beyond a unit test (>= 32 tiles of 256x256, or >= 1024 k-tiles), but
    the forced 256x256 tile (hints 4 and 4 | 1024) takes the TN split-K cases there; the grouped use of the same kernel (gemm_wg.hip's
    256x256 tile inside cmda_gemm_grouped) is what test_exact_deferred_grouped_weight_gradients runs.
    The cap on refusals is part of the test: more than a quarter of the launches refused means the cases no longer test the library."""
    walked = [test_exact_plain_layouts, test_exact_plain_epilogues_strides_alignment, test_exact_split_k_atomics, test_exact_batched_heads,
              test_exact_conv_views, test_exact_reflect_padded_view, test_exact_input_dilated_view_strided_dgrad,
              test_exact_transposed_convolution, test_exact_permuted_weight_gradient_store, test_exact_unpatchify_store,
              test_exact_fused_column_statistics, test_exact_split_bf16_low_halves, test_exact_split_bf16_low_halves_three_launch_path]
    for c in (PLANS, TALLY, REFUSED):
        c.clear()
    saved = (ops.GEMM_TILE_HINT, ops.X3_BIG_FLOPS, ops.X3_BIG_INTENSITY)
    PLAN_ONLY[0] = True
    try:
        for fn in walked:
            for kw in _cases_of(fn):
                try:
                    fn(tgt, **kw)
                finally:
                    ops.GEMM_TILE_HINT, ops.X3_BIG_FLOPS, ops.X3_BIG_INTENSITY = saved
    finally:
        PLAN_ONLY[0] = False
    print(f'\n{tgt.kind}: {TALLY["ran"]} launches, {TALLY["refused"]} refused')
    for (fam, tile, stages, waves), n in sorted(PLANS.items()):
        print(f'  {FAMILY[fam]:9s} {TILE[tile]:8s} {stages} stages {waves} waves: {n}')
    for (what, mode), n in sorted(REFUSED.items()):
        print(f'  refused: {what}, mode {mode}: {n}')
    families = {FAMILY[k[0]] for k in PLANS}
    assert families >= {'PINGPONG', 'WGRAD', 'GLDS', 'LEAN', 'REG', 'X3REG', 'X3LEAN'}, f'families reached: {sorted(families)}'
    tiles = {TILE[k[1]] for k in PLANS}
    assert tiles == set(TILE), f'tiles reached: {sorted(tiles)}'
    for fam in ('GLDS', 'LEAN'):
        stages = {k[2] for k in PLANS if FAMILY[k[0]] == fam}
        assert stages >= {2, 4}, f'{fam}: LDS-DMA stage counts reached: {sorted(stages)}'
    share = TALLY['refused'] / (TALLY['ran'] + TALLY['refused'])
    assert share <= 0.25, f'{TALLY["refused"]} of {TALLY["ran"] + TALLY["refused"]} launches refused'
