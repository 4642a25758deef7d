"""Thin tensor-level wrappers over the C ABI (include/cmda_hip.h).  No autograd here: the
differentiable building blocks live in cmda_amd/functional.py and call these for both passes."""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from . import deferred as D
from ._lib import BF16, F32, GemmParams, View, c_f32, c_i32, c_i64, call, check_dev, dtype_tag, ptr, stream_of

_ESIZE = {torch.float32: 4, torch.bfloat16: 2}


def _chunk(t):
    return 16 // _ESIZE[t.dtype]


def plain_view(t, rows, cols, ld=None, batch_stride=0, offset=0, batch2_stride=0):
    """View of a row-major matrix living inside tensor `t` (element `offset` from its start)."""
    ld = cols if ld is None else ld
    es = _ESIZE[t.dtype]
    ch = 16 // es
    base = t.data_ptr() + offset * es
    vec_ok = int(base % 16 == 0 and ld % ch == 0 and batch_stride % ch == 0 and batch2_stride % ch == 0)
    v = View(ptr=base, ld=ld, R=rows, Cc=cols, batch_stride=batch_stride, batch2_stride=batch2_stride, conv=0,
             vec_ok=vec_ok,
             H=0, W=0, C=1, OH=1, OW=1, KH=1, KW=1, stride=1, pad=0, dil=1, in_dil=1, reflect=0)
    v._t, v._off = t, offset    # (the tensor behind the view: `_gemm_x3_big` re-points the view at its bf16 hi / lo copies)
    return v


def conv_view(x, B, H, W, C, KH, KW, stride, pad, dil=1, OH=None, OW=None, in_dil=1, reflect=0):
    """im2col view of NHWC tensor x[B,H,W,C]: r=(b,oh,ow), c=(kh,kw,ci)."""
    if OH is None:
        OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
        OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    ch = _chunk(x)
    vec_ok = int(x.data_ptr() % 16 == 0 and C % ch == 0)
    # non-overlapping patches (the spatial-reduction convolutions): the same matrix, but its rows / K segments are contiguous
    # runs the kernels can fill like a plain operand (conv = 2)
    patch = (KH == KW == stride and pad == 0 and dil == 1 and in_dil == 1 and not reflect and H == OH * stride and W == OW * stride)
    v = View(ptr=x.data_ptr(), ld=0, R=B * OH * OW, Cc=KH * KW * C, batch_stride=0, batch2_stride=0, conv=2 if patch else 1, H=H, W=W, C=C,
             OH=OH, OW=OW, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil, in_dil=in_dil, reflect=reflect,
             vec_ok=vec_ok)
    v._t, v._off = x, 0
    return v


ACT = {None: 0, 'none': 0, 'relu': 1, 'gelu': 2, 'tanh': 3}

# bench.py's roofline leg: when a list is installed here every GEMM launch is bracketed by events on the launch stream
GEMM_PROFILE = None
# which part of the path is issuing work (set by the modules through `site(...)`): bench.py splits the MFMA roofline by it --
# 'mit' (the MiT encoders: the blocks the 0.60 target is defined on), 'fusion', 'head', 'generator', 'other'
GEMM_SITE = 'other'


class site:
    """with ops.site('mit'): ...  -- tags every GEMM / fused-attention launch (and every queued weight gradient) issued inside"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global GEMM_SITE
        self.prev, GEMM_SITE = GEMM_SITE, self.name

    def __exit__(self, *exc):
        global GEMM_SITE
        GEMM_SITE = self.prev


def sited(name):
    """decorator form of `site`"""
    def deco(fn):
        import functools

        @functools.wraps(fn)
        def wrapped(*a, **k):
            with site(name):
                return fn(*a, **k)
        return wrapped
    return deco


def _attn_profile(flops, fn):
    """bench.py's roofline leg: bracket a fused-attention launch like a GEMM launch (MFMA work of the MiT blocks)"""
    if GEMM_PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    GEMM_PROFILE.append((flops, e0, e1, 0, ('attention', GEMM_SITE)))
    return r
# cmda_gemm_params_t.tile_hint for every GEMM issued from here (0 = the library's heuristics); set by tuning sweeps / tests
GEMM_TILE_HINT = int(os.environ.get('CMDA_GEMM_TILE_HINT', '0'))   # cmda_gemm_params_t.tile_hint of every launch (tuning sweeps, forced-tile tests)


# ---- split-bf16 mode, LARGE problems: three launches of the bf16 kernels over operands split once in HBM -------------------------
# The register-staged split kernel (csrc/gemm_x3.hip) runs the decode head's 3 x 3 bottleneck at ~170 TFLOP/s (7.3 ms per call at
# 16 images) where the bf16 LDS-DMA kernel does 1.1 PFLOP/s; x = hi + lo with both halves stored as bf16 tensors of x's own layout
# turns the contraction into a_lo b_hi + a_hi b_lo + a_hi b_hi on that kernel, accumulated in the fp32 output (beta = 1 / atomics):
# same ~16 mantissa bits per product, 8 bytes of extra traffic per operand element.
X3_BIG_FLOPS = float(os.environ.get('CMDA_X3_BIG_GFLOP', '15')) * 1e9   # (bench, ms per step at 40 / 20 / 10 / 5 / 2 GFLOP: 149.2 / 144.7 / 145.1 / 150.7 / 162.3)


def split_bf16(t):
    """(hi, lo) bf16 tensors of t's shape: hi = bf16(t), lo = bf16(t - hi).  Nothing is cached: a captured iteration replays the
    split launch with that iteration's operand values (the weights of these problems are a few MB)."""
    check_dev(t)
    hi = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    lo = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    call('cmda_split_bf16', ptr(t), ptr(hi), ptr(lo), c_i64(t.numel()), stream_of(t))
    return hi, lo


X3_BIG_INTENSITY = float(os.environ.get('CMDA_X3_BIG_INTENSITY', 100))   # FLOP per byte moved by the split / accumulate passes


def _x3_big_ok(A, B, out, M, N, K, nb, act, rowscale, hold, defer, splits, c_patch, c_perm):
    if hold or act is not None or rowscale is not None or c_patch is not None or GEMM_TILE_HINT != 0:
        return False
    if 2.0 * M * N * K * nb < X3_BIG_FLOPS or out.dtype != torch.float32:
        return False
    moved = 16.0 * M * N * nb   # two more read + write passes over the fp32 output (beta = 1 launches)
    for v in (A, B):
        t = getattr(v, '_t', None)
        if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() % 8 or t.data_ptr() % 16:
            return False
        if v.conv:
            if v.C % 8:
                return False
        elif v.ld % 8 or v._off % 8 or v.batch_stride % 8 or v.batch2_stride % 8:
            return False
        moved += 12.0 * t.numel()   # the split pass: 4 bytes read, 2 x 2 written, the halves read again
    # the three launches pay for themselves where the contraction outweighs those passes (profiles/r05_x3_gemm.txt: 4096^3 at 204 FLOP
    # per moved byte 460 against 728 us on the register-staged split kernel; the head's pointwise convolution 262144 x 256 x 1024 at 32:
    # 1438 against 1119)
    return 2.0 * M * N * K * nb >= X3_BIG_INTENSITY * moved


def _x3_half_views(v):
    hi, lo = split_bf16(v._t)
    out = []
    for h in (hi, lo):
        w = View.from_buffer_copy(bytes(v))
        w.ptr = h.data_ptr() + v._off * 2
        w.vec_ok = 1
        w._t, w._off = h, v._off
        out.append(w)
    return out[0], out[1], (hi, lo)


def _gemm_x3_big(A, B, out, M, N, K, kw, colstats=None):
    """out = a_lo b_hi + a_hi b_lo + a_hi b_hi (bias / residual / caller's beta in the first launch; fused column statistics in the
    last one, whose epilogue stores the final values)"""
    a_hi, a_lo, ka = _x3_half_views(A)
    b_hi, b_lo, kb = _x3_half_views(B)
    keep = tuple(kw.pop('keep', ())) + ka + kb
    first = dict(kw)
    rest = dict(kw, bias=None, res=None)
    atomic = kw.get('atomic', False)
    if not atomic:
        rest['beta'] = 1.0
    colsum = kw.get('colsum')
    # the bias gradient (column sums of A = dy): sum of the two halves' column sums, taken in the launches that read them first
    gemm(a_lo, b_hi, out, M, N, K, **dict(first, dtype=1, colsum=colsum, keep=keep))
    gemm(a_hi, b_lo, out, M, N, K, **dict(rest, dtype=1, colsum=colsum, keep=keep))
    gemm(a_hi, b_hi, out, M, N, K, **dict(rest, dtype=1, colsum=None, keep=keep, colstats=colstats))
    return out


def gemm(A, B, out, M, N, K, *, a_kstrided=False, b_kstrided=False, ldc=None, batch=1, c_batch_stride=0,
         batch2=1, c_batch2_stride=0, res_batch2_stride=0, splits=1, alpha=1.0, beta=0.0, bias=None, act=None, res=None, ldres=None, res_batch_stride=0,
         rowscale=None, rows_per_scale=1, atomic=False, dtype=None, c_offset=0, colsum=None, c_patch=None, c_perm=None, defer=False, keep=(),
         hold=False, colstats=None):
    """out[m,n] = epi(alpha * sum_k A(m,k) B(n,k)); A/B are `View`s built by plain_view / conv_view.
    defer=True (weight gradients: nothing reads `out` before the pass ends): inside a `backward_scope` the launch is only QUEUED
    and goes out with the next `gemm_flush_deferred()` as part of a grouped launch; `keep` = the tensors behind the operand views
    (kept alive until then).
    hold=True: build the problem but do NOT launch it -- returns (params, meta, out, keep) for tools that time or inspect it.
    colstats=(ws, rows_per_group): column sums / sums of squares of the stored output accumulated into the BatchNorm workspace `ws`
    (`bn_stats_ws`: zero on entry) by the epilogue -- the statistics pass of the BatchNorm / InstanceNorm behind this convolution
    (`colstats_ok` says whether a problem qualifies)."""
    check_dev(out, bias, res, rowscale)
    if dtype == 2 and _x3_big_ok(A, B, out, M, N, K, batch * batch2, act, rowscale, hold, defer, splits, c_patch, c_perm):
        return _gemm_x3_big(A, B, out, M, N, K, dict(a_kstrided=a_kstrided, b_kstrided=b_kstrided, ldc=ldc, batch=batch,
                                                     c_batch_stride=c_batch_stride, batch2=batch2, c_batch2_stride=c_batch2_stride,
                                                     res_batch2_stride=res_batch2_stride, splits=splits, alpha=alpha, beta=beta, bias=bias,
                                                     res=res, ldres=ldres, res_batch_stride=res_batch_stride, atomic=atomic,
                                                     c_offset=c_offset, colsum=colsum, c_perm=c_perm, defer=defer, keep=keep), colstats=colstats)
    out_f32 = out.dtype == torch.float32
    p = GemmParams()
    p.A, p.B = A, B
    p.a_kstrided, p.b_kstrided = int(a_kstrided), int(b_kstrided)
    p.C = out.data_ptr() + c_offset * _ESIZE[out.dtype]
    p.ldc = N if ldc is None else ldc
    p.c_batch_stride, p.c_batch2_stride = c_batch_stride, c_batch2_stride
    p.M, p.N, p.K, p.batch, p.batch2, p.splits = M, N, K, batch, batch2, splits
    p.alpha, p.beta = alpha, beta
    p.bias = bias.data_ptr() if bias is not None else None
    p.act = ACT[act]
    p.res = res.data_ptr() if res is not None else None
    p.res_f32 = int(res is not None and res.dtype == torch.float32 and dtype == 1)   # fp32 residual stream of the bf16 mode
    p.ldres = (N if ldres is None else ldres)
    p.res_batch_stride, p.res_batch2_stride = res_batch_stride, res_batch2_stride
    p.rowscale = rowscale.data_ptr() if rowscale is not None else None
    p.rows_per_scale = rows_per_scale
    p.dtype = dtype
    p.out_f32 = int(out_f32)
    assert out_f32 or not atomic
    p.atomic = int(atomic)
    ok = (p.ldc % 4 == 0 and c_batch_stride % 4 == 0 and c_batch2_stride % 4 == 0 and p.C % 16 == 0)
    if res is not None:
        ok = ok and p.ldres % 4 == 0 and res_batch_stride % 4 == 0 and res_batch2_stride % 4 == 0 and res.data_ptr() % 16 == 0
    if bias is not None:
        ok = ok and bias.data_ptr() % 16 == 0
    p.c_vec_ok = int(ok)
    p.colsum = colsum.data_ptr() if colsum is not None else None
    if colstats is not None:
        check_dev(colstats[0])
        assert colstats[0].dtype == torch.float32 and not defer and not atomic
        p.colstats, p.colstats_rows = colstats[0].data_ptr(), colstats[1]
    p.tile_hint = GEMM_TILE_HINT
    if c_perm is not None:   # (Ci, KH*KW): atomic store of a conv weight gradient in the parameter's [Co,Ci,KH,KW] layout
        assert atomic and batch == 1 and batch2 == 1
        p.c_perm_ci, p.c_perm_cells = c_perm
    if c_patch is not None:  # (OW, KH, KW*Ci): store rows (b,oh,ow) x cols (kh,kw,ci) un-patchified into NHWC
        assert res is None and batch == 1 and batch2 == 1 and not atomic
        p.c_patch_ow, p.c_patch_kh, p.c_patch_kwci = c_patch
        p.c_vec_ok = int(p.C % 16 == 0 and c_patch[2] % 4 == 0 and (bias is None or bias.data_ptr() % 16 == 0))
    if defer:
        # deferred problems are launched AFTER the grouped ones of their flush whatever their list position (cmda_gemm_grouped): only
        # commutative accumulation may be deferred
        assert atomic and beta == 0.0, 'ops.gemm(defer=True) is for atomic accumulation only'
    if defer and D.depth > 0 and GEMM_DEFER:
        es = 2 if dtype == 1 else 4
        nb = batch * batch2
        D.enqueue((p, (out, colsum) + tuple(keep), 2.0 * M * N * K * nb, (M * K + N * K) * nb * es + 2 * M * N * nb * 4, GEMM_SITE))
        return out
    if hold or (GEMM_PROFILE is not None and out.is_cuda):
        es = 2 if dtype == 1 else 4
        nb = batch * batch2

        def _unique(v):  # bytes of the tensor behind an operand view (an im2col view re-reads, the tensor is counted once)
            return (v.R // max(1, v.OH * v.OW) * v.H * v.W * v.C if v.conv else v.R * v.Cc * nb) * es
        cbytes = M * N * nb * (4 if out_f32 else es) * (2 if (atomic or beta != 0.0) else 1)
        meta = (2.0 * M * N * K * nb, _unique(A) + _unique(B) + cbytes + (M * N * nb * es if res is not None else 0),
                (M, N, K, nb, splits, bool(A.conv or B.conv), bool(a_kstrided), bool(b_kstrided), bool(atomic), out_f32))
        if hold:
            return (p, meta, out, (bias, res, rowscale, colsum) + tuple(keep))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call('cmda_gemm', ctypes.byref(p), stream_of(out))
        e1.record()
        GEMM_PROFILE.append((meta[0], e0, e1, meta[1], meta[2] + (GEMM_SITE,)))
        return out
    call('cmda_gemm', ctypes.byref(p), stream_of(out))
    return out


# ---- deferred weight gradients: queued by gemm(defer=True) inside a backward scope, launched in groups (cmda_gemm_grouped) -----
GEMM_DEFER = os.environ.get('CMDA_GEMM_DEFER', '1') != '0'    # False: defer=True launches in place (A/B switch for tuning, tests of the single-launch path)


def run_tail(key):
    """launch everything postponed under `key` (deferred.queue_under): the closures, then the queued weight gradients"""
    for fn in D.TAIL.pending.pop(key, ()):
        fn()
    gemm_flush_deferred(from_lane=key)


def gemm_flush_deferred(all_lanes=False, from_lane=None):
    """launch what gemm(defer=True) queued since the last flush: the CURRENT concurrency lane's queue by default (another lane's
    producers may still be running on their stream), every queue with all_lanes (after the lanes were joined).  from_lane: launch
    THAT lane's queue from here (a side lane entered behind the producers: the decode head's weight gradients next to the encoders'
    backward pass, segmentors.train_bwd)."""
    lane = from_lane if from_lane is not None else (None if all_lanes else D.LANES[-1])
    for key in D.select(D.GEMM.pending, lane):
        q = D.GEMM.pending.pop(key, None)
        if not q:
            continue
        n = len(q)
        arr = (GemmParams * n)(*[e[0] for e in q])
        out0 = q[0][1][0]
        plan, upload = D.gemm_plan((str(out0.device), bytes(arr)), out0.device,
                                   lambda: int(L.lib().cmda_gemm_grouped_ws_bytes(arr, c_i32(n))))
        host, devbuf, nbytes = plan[:3]
        prof = GEMM_PROFILE is not None and out0.is_cuda
        if prof:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        call('cmda_gemm_grouped', arr, c_i32(n), ptr(host), ptr(devbuf), c_i64(nbytes), c_i32(upload), stream_of(out0))
        if prof:
            e1.record()
            split = {}
            for e in q:
                split[e[4]] = split.get(e[4], 0.0) + e[2]
            GEMM_PROFILE.append((sum(e[2] for e in q), e0, e1, sum(e[3] for e in q), ('grouped', n, 0, 0, 0, False, True, True, True, True, split)))


def layernorm_fwd(x, gamma, beta, eps, save_stats=True, out=None, out_dtype=None):
    """y = LayerNorm(x); y takes out's dtype, else out_dtype, else x's (x fp32 -> y bf16 and back: the fp32 residual stream)"""
    check_dev(x, gamma, beta, out)
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device) if out is None else out
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    call('cmda_layernorm_fwd2', ptr(x), dtype_tag(x), ptr(gamma), ptr(beta), ptr(y), dtype_tag(y), ptr(mean), ptr(rstd), c_i64(rows),
         c_i32(C), c_f32(eps), stream_of(x))
    return y, mean, rstd


class backward_scope:
    """A backward pass: inside it the LayerNorm parameter gradients, the conv weight-gradient shadows, the weight-gradient GEMMs and
    the tail closures are deferred (flush_deferred launches them).  The outermost exit, which follows the lanes' joins, launches
    what is left on every lane -- or drops it when the pass raised."""

    def __enter__(self):
        D.depth += 1
        return self

    def __exit__(self, *exc):
        D.depth -= 1
        if D.depth == 0:
            if exc[0] is None:
                for key in list(D.TAIL.pending):   # (a tail nobody ran: run it here)
                    for fn in D.TAIL.pending.pop(key):
                        fn()
                flush_deferred(all_lanes=True)
            else:   # the pass died half way: drop what it queued / touched instead of folding it into the next pass
                D.reset()
        return False


def _ln_fold_plan(dev, regions):
    desc = np.zeros(len(regions), dtype=[('ws', '<u8'), ('dg', '<u8'), ('db', '<u8'), ('C', '<i4'), ('n', '<i4')])
    for i, (ws, dg, db, C, nslots) in enumerate(regions):
        desc[i] = (ws.data_ptr(), dg.data_ptr(), db.data_ptr(), C, nslots)
    return D.host_table(desc, dev), len(regions), max(r[3] for r in regions)


def _conv_drain_plan(dev, shadows):
    desc = np.zeros(len(shadows), dtype=[('src', '<u8'), ('dst', '<u8'), ('d', '<i4', 4), ('p', '<i4', 4), ('flip', '<i4'),
                                         ('mode', '<i4'), ('total', '<i8')])
    blocks = []
    for i, (sh, g) in enumerate(shadows):
        Co, Ci, KH, KW = g.shape
        cs = sh.shape[1] // (KH * KW)   # channels of the shadow (> Ci: padded)
        desc[i] = (sh.data_ptr(), g.data_ptr(), (Co, KH, KW, cs), (0, 3, 1, 2), ((4 << 8) | (Ci << 16)) if cs != Ci else 0, 2, g.numel())
        blocks += [(i, b) for b in range((g.numel() + 1023) // 1024)]
    return D.host_table(desc, dev), D.host_table(np.asarray(blocks, dtype=np.int32), dev), len(blocks)


def flush_deferred(all_lanes=False):
    """launch the queued weight gradients, then drain the conv shadows and fold the LayerNorm partial sums (one launch per device
    each).  Only the CURRENT concurrency lane's work by default: another lane's kernels may still be running on their stream."""
    lane = None if all_lanes else D.LANES[-1]
    gemm_flush_deferred(all_lanes)   # queued weight gradients first: the convolution ones land in the shadows drained next
    for (tab, blk, nblocks), t in D.launch_plans(D.CONV, lane, _conv_drain_plan):
        call('cmda_permute4_batch', ptr(tab), ptr(blk), c_i32(nblocks), stream_of(t))
    for (tab, n, max_c), t in D.launch_plans(D.LN, lane, _ln_fold_plan):
        call('cmda_layernorm_fold_batch', ptr(tab), c_i32(n), c_i32(max_c), stream_of(t))


# Deferred convolution weight gradients: inside a backward scope a conv weight gradient is accumulated by the GEMM's atomics in the
# GEMM's own column order (kh, kw, ci) -- coalesced -- into a persistent zeroed fp32 shadow [Co,KH,KW,Ci] of the parameter's
# gradient, and ONE batched launch per flush moves all shadows into the [Co,Ci,KH,KW] gradients and clears them (the permuted
# atomic store it replaces cost 20-84 us per spatial-reduction conv against 10-14 us, tools/dbg/srconv_dbg.py).
def conv_grad_shadow(grad, ci_pad=0):
    """grad: fp32 [Co,Ci,KH,KW] parameter gradient -> its [Co, KH*KW*Ci] shadow, or None outside a backward scope.  ci_pad > Ci:
    the shadow carries the padded channels of the GEMM ([Co, KH*KW*ci_pad]); the drain keeps the real ones."""
    Co, Ci, KH, KW = grad.shape
    if ci_pad <= Ci and not grad.is_contiguous() and grad.permute(0, 2, 3, 1).is_contiguous():
        # channels-last stored gradient (optim.FlatAdamW): its memory is the GEMM's own [Co][KH][KW][Ci] order -- accumulate in place,
        # nothing to drain
        return grad.permute(0, 2, 3, 1).reshape(Co, KH * KW * Ci)
    if D.depth == 0:
        return None
    return D.conv_shadow(grad, KH * KW * max(Ci, ci_pad))


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dres=None, out_scale=None, rows_per_scale=0):
    """returns dx, or (dx, dx * out_scale[row // rows_per_scale]) when a per-sample scale is given (DropPath of the consumer)"""
    check_dev(dy, x, gamma, mean, rstd, dgamma, dbeta, dres, out_scale)
    C = x.shape[-1]
    rows = x.numel() // C
    dx = torch.empty_like(dy)       # (x may be the fp32 residual stream while the gradients travel in the compute dtype)
    dxs = torch.empty_like(dy) if out_scale is not None else None
    if D.depth > 0:   # (backward scope: partial sums into the layer's region, folded by flush_deferred)
        ws, dg, db = D.ln_region(dgamma, dbeta, C), None, None
    else:
        ws, dg, db = D.workspace('ln', x.device, L.lib().cmda_layernorm_bwd_ws_floats(rows, C)), dgamma, dbeta
    call('cmda_layernorm_bwd2', ptr(dy), ptr(x), dtype_tag(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dg),
         ptr(db), ptr(ws), c_i64(rows), c_i32(C), ptr(out_scale), c_i64(rows_per_scale), ptr(dxs), dtype_tag(dy), stream_of(x))
    return dx if out_scale is None else (dx, dxs)


def permute4(src, dst, dims, perm, flipmask=0, accumulate=False):
    """dst (contiguous, dims[perm]) = permute(src viewed as `dims`), with optional axis flips / accumulate."""
    check_dev(src, dst)
    d = list(dims) + [1] * (4 - len(dims))
    p = list(perm) + list(range(len(perm), 4))
    call('cmda_permute4', ptr(src), ptr(dst), *[c_i32(v) for v in d], *[c_i32(v) for v in p], c_i32(flipmask),
         c_i32(int(accumulate)), dtype_tag(src), dtype_tag(dst), stream_of(src))
    return dst


def conv_co1_ok(x, C, K, pad):
    return x.dtype in (torch.bfloat16, torch.float32) and C == 64 and K == 7 and pad == 3


def conv_co1(x, w, bias, B, H, W, C, K, pad, reflect, act):
    """x [B*H*W, C] NHWC, w [K*K*C] khwc (activation dtype) -> fp32 [B,H,W] = act(bias + conv): one output channel"""
    check_dev(x, w, bias)
    out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    call('cmda_conv_co1', ptr(x), ptr(w), ptr(bias), ptr(out), c_i32(B), c_i32(H), c_i32(W), c_i32(C), c_i32(K), c_i32(pad),
         c_i32(int(reflect)), c_i32(ACT[act]), dtype_tag(x), stream_of(x))
    return out


def conv_co3(x, w, bias, B, H, W, C, K, pad, reflect, act, scale=None, shift=None):
    """x [B*H*W, C] NHWC, w [3, K*K*C] khwc (activation dtype) -> fp32 NCHW [B,3,H,W] = act(bias + conv) * scale + shift (per output
    channel; scale / shift fp32 [3] or both None): three output channels (conv_co1_ok decides the shapes)"""
    check_dev(x, w, bias, scale, shift)
    if (scale is None) != (shift is None):
        raise L.CmdaError('conv_co3: scale and shift go together')
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    call('cmda_conv_co3', ptr(x), ptr(w), ptr(bias), ptr(scale), ptr(shift), ptr(out), c_i32(B), c_i32(H), c_i32(W), c_i32(C), c_i32(K),
         c_i32(pad), c_i32(int(reflect)), c_i32(ACT[act]), dtype_tag(x), stream_of(x))
    return out


def cast_pad_cols(src32, cp, dtype):
    """fp32 [rows, c] -> dtype [rows, cp], columns >= c zero"""
    check_dev(src32)
    rows, c = src32.shape
    dst = torch.empty(rows, cp, dtype=dtype, device=src32.device)
    call('cmda_cast_pad_cols', ptr(src32), ptr(dst), c_i64(rows), c_i32(c), c_i32(cp), dtype_tag(dst), stream_of(src32))
    return dst


def rows_fill(out, bias):
    """out fp32 [rows, C] = bias[C] broadcast (zeros when bias is None)"""
    check_dev(out, bias)
    call('cmda_rows_fill', ptr(out), ptr(bias), c_i64(out.shape[0]), c_i32(out.shape[1]), stream_of(out))
    return out


def nchw_to_nhwc_pad(src, dst, B, C, HW, cpad):
    """src fp32 NCHW [B,C,H,W] -> dst [B*HW, cpad] (activation dtype), channels >= C zero"""
    check_dev(src, dst)
    call('cmda_nchw_to_nhwc_pad', ptr(src), ptr(dst), c_i32(B), c_i32(C), c_i64(HW), c_i32(cpad), dtype_tag(dst), stream_of(src))
    return dst


def permute4_batch(desc, blocks, nblocks):
    """desc: DEVICE uint8 tensor holding an array of cmda_permute_desc_t; blocks: DEVICE int32 [nblocks, 2]"""
    check_dev(desc, blocks)
    call('cmda_permute4_batch', ptr(desc), ptr(blocks), c_i32(nblocks), stream_of(desc))


def zero_ws(device, n):
    """persistent fp32 accumulation workspace, ZERO on entry by contract: whoever accumulates into it drains it with cast_clear
    (one buffer per device and concurrency lane: deferred.workspace)"""
    return D.workspace('zero', device, n)[:n]


def cast_clear(src32, dtype):
    """returns src32 cast to `dtype` and zeroes src32 (one launch)"""
    check_dev(src32)
    dst = torch.empty(src32.shape, dtype=dtype, device=src32.device)
    call('cmda_cast_clear', ptr(src32), ptr(dst), c_i64(src32.numel()), dtype_tag(dst), stream_of(src32))
    return dst


def cast(src, dtype):
    if src.dtype == dtype:
        return src
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    return permute4(src, dst, (src.numel(), 1, 1, 1), (0, 1, 2, 3))


def colsum(x, out, M, N, ld=None, offset=0):
    """out[N] += column sums of the [M,N] matrix at element `offset` of x with row pitch ld."""
    check_dev(x, out)
    call('cmda_colsum', L.c_vp(x.data_ptr() + offset * _ESIZE[x.dtype]), ptr(out), c_i64(M), c_i32(N),
         c_i64(N if ld is None else ld), dtype_tag(x), stream_of(x))
    return out


def axpby(x, y, a, b, out=None):
    check_dev(x, y)
    out = torch.empty_like(x) if out is None else out
    call('cmda_axpby', ptr(x), ptr(y), ptr(out), c_f32(a), c_f32(b), c_i64(x.numel()), dtype_tag(x), stream_of(x))
    return out


def ema_update(ema, param, alpha, mirror=None):
    """ema = alpha * ema + (1 - alpha) * param; mirror: optional bf16 tensor of the same length that receives the result too"""
    check_dev(ema, param, mirror)
    call('cmda_ema_update', ptr(ema), ptr(param), c_f32(alpha), c_i64(ema.numel()), ptr(mirror), stream_of(ema))


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, p_bf16=None):
    check_dev(p, g, m, v, p_bf16)
    call('cmda_adamw_step', ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), c_i64(p.numel()), c_f32(lr), c_f32(beta1),
         c_f32(beta2), c_f32(eps), c_f32(wd), c_i32(step), stream_of(p))


def class_mix(src, tgt, src_label, classes, channels_last=False):
    """src/tgt [B,C,H,W] (or [B,H,W,C]); src_label int64 [B,H,W]; classes int64 [B,K] padded with -1."""
    check_dev(src, tgt, src_label, classes)
    out = torch.empty_like(src)
    B = src.shape[0]
    HW = src_label.shape[-2] * src_label.shape[-1]
    Cch = src.numel() // (B * HW)
    call('cmda_class_mix', ptr(src), ptr(tgt), ptr(out), ptr(src_label), ptr(classes), c_i32(classes.shape[1]), c_i32(B),
         c_i32(HW), c_i32(Cch), c_i32(int(channels_last)), dtype_tag(src), stream_of(src))
    return out


def class_mix_label(src, tgt, src_label, classes):
    check_dev(src, tgt, src_label, classes)
    out = torch.empty_like(src)
    B = src.shape[0]
    call('cmda_class_mix_label', ptr(src), ptr(tgt), ptr(out), ptr(src_label), ptr(classes), c_i32(classes.shape[1]),
         c_i32(B), c_i32(src.numel() // B), stream_of(src))
    return out


def softmax_fwd_(s, rows, L, alpha):
    check_dev(s)
    call('cmda_softmax_fwd', ptr(s), c_i64(rows), c_i32(L), c_f32(alpha), dtype_tag(s), stream_of(s))
    return s


def softmax_bwd_(p, dp, rows, L, alpha):
    check_dev(p, dp)
    call('cmda_softmax_bwd', ptr(p), ptr(dp), c_i64(rows), c_i32(L), c_f32(alpha), dtype_tag(p), stream_of(p))
    return dp


# Wide heads (head dim > 64: the fusion modules' single-head Blocks) that take the chunked fused kernels of attention_wide.hip BY DEFAULT,
# one entry per head dim of the two reference configs: (forward only, forward + backward).  Set from tools/attn_bench.py on the MI355X
# (profiles/attn_wide_bench.txt): the kernels walk the head dim serially, ~2.3 us per 64-wide tile, and the fusion blocks' shapes give them
# 8 ... 512 workgroups, so the walk wins where it is short -- fused / unfused at the configs' shapes: 128 fwd 0.32-0.51, fwd + bwd
# 0.74-0.91; 256 fwd 0.87, fwd + bwd 1.30; 320 1.02 / 1.16; 512 1.53 / 1.63; 640 1.88 / 2.09; 1024 2.83 / 2.84.  A head dim that is slower
# stays on the GEMM + softmax path; so does one that is not listed (not measured).
ATTN_WIDE_TABLE = {128: (True, True), 256: (True, False), 320: (False, False), 512: (False, False), 640: (False, False),
                   1024: (False, False)}


def attention_fused_ok(q, Nk, heads, C, need_grad=True, x3=False):
    """the fused kernels hold every key of a (batch, head) in LDS: up to 256 with a backward pass to follow, up to 320 forward-only
    (inference on 440 x 640 frames: 260 / 280 keys, encoder_decoder.py:897-936).  x3: the split-bf16 mode (fp32 storage, runtime.gemm_x3)
    has instances of its own -- K / V as hi + lo bf16 images in LDS, up to 256 keys.  bf16 heads wider than 64 (multiples of 64 up to
    1024) have the chunked instances; CMDA_ATTN_WIDE, read at call time (same-process A/B): unset / 1 = those ATTN_WIDE_TABLE names,
    0 = none (GEMM + softmax), 2 = every wide head whatever the table says (kernel tests, tools/attn_bench.py)"""
    if x3 and q.dtype == torch.float32:
        return C == heads * 64 and 0 < Nk <= 256 and not ATTN_X3_OFF
    if q.dtype != torch.bfloat16 or heads <= 0 or C % heads or not 0 < Nk <= (256 if need_grad else 320):
        return False
    hd = C // heads
    if hd == 64:
        return True
    mode = os.environ.get('CMDA_ATTN_WIDE', '1')
    if hd % 64 or not 64 < hd <= 1024 or mode == '0':
        return False
    return mode == '2' or ATTN_WIDE_TABLE.get(hd, (False, False))[1 if need_grad else 0]


ATTN_X3_OFF = os.environ.get('CMDA_ATTN_X3', '1') == '0'   # split-bf16 mode on the unfused GEMM + softmax path (same-box A/B)


def _kv_split(kv):
    """hi / lo bf16 halves of an fp32 kv tensor, split ONCE per attention call (cmda_split_bf16) and kept on the tensor for the
    backward pass, which reads the same kv"""
    pair = getattr(kv, '_cmda_split', None)
    if pair is None or pair[2] != kv._version:
        hi, lo = split_bf16(kv)
        pair = kv._cmda_split = (hi, lo, kv._version)
    return pair[0], pair[1]


def attention_fused_fwd(q, kv, B, N, Nk, heads, C, scale):
    check_dev(q, kv)
    o = torch.empty(B * N, C, dtype=q.dtype, device=q.device)
    if q.dtype == torch.float32:   # split-bf16 instances (fp32 storage)
        hi, lo = _kv_split(kv)
        _attn_profile(4.0 * B * N * Nk * C, lambda: call('cmda_attention_fwd_x3', ptr(q), ptr(hi), ptr(lo), ptr(o), c_i32(B), c_i32(N),
                                                         c_i32(Nk), c_i32(heads), c_i32(C), c_f32(scale), stream_of(q)))
        return o
    _attn_profile(4.0 * B * N * Nk * C, lambda: call('cmda_attention_fwd', ptr(q), ptr(kv), ptr(o), c_i32(B), c_i32(N), c_i32(Nk),
                                                     c_i32(heads), c_i32(C), c_f32(scale), dtype_tag(q), stream_of(q)))
    return o


def attention_fwd_queries_per_block(B, N, heads, Nk=256, scale=0.125):
    """queries per block of the forward and dQ kernels at head dim 64 (bf16): the rule of fwd_queries_per_block in attention.hip,
    restated for the tools that label their timings with it (tools/dbg/attn_graph_bench.py) -- the library does not export it.
    The full-key instances (256 keys, scale > 0) switch to 128 from 512 blocks of 128 up, the masked ones from 1024"""
    full = int(Nk) == 256 and scale > 0
    return 64 if -(-int(N) // 128) * int(heads) * int(B) < (512 if full else 1024) else 128


def attention_bwd_direct(B, N, Nk, heads):
    """True: the fused backward stores dK | dV straight as bf16 (few queries: one block per key slice walks them all)"""
    return bool(L.lib().cmda_attention_bwd_direct(int(B), int(N), int(Nk), int(heads)))


def attention_fused_bwd(q, kv, do, dkv32, B, N, Nk, heads, C, scale, dkv16=None):
    """returns dq; dK | dV accumulate into dkv32 (fp32 [B*Nk, 2C], zero on entry) or -- direct mode -- are stored into dkv16 (bf16)"""
    check_dev(q, kv, do, dkv32, dkv16)
    dq = torch.empty(B * N, C, dtype=q.dtype, device=q.device)
    stats = torch.empty(B * N * heads * 2, dtype=torch.float32, device=q.device)
    if q.dtype == torch.float32:   # split-bf16 instances: `dkv16` is then the fp32 dK | dV tensor of the direct mode
        hi, lo = _kv_split(kv)
        _attn_profile(10.0 * B * N * Nk * C, lambda: call('cmda_attention_bwd_x3', ptr(q), ptr(hi), ptr(lo), ptr(do), ptr(dq), ptr(dkv32),
                                                          ptr(dkv16), ptr(stats), c_i32(B), c_i32(N), c_i32(Nk), c_i32(heads), c_i32(C),
                                                          c_f32(scale), stream_of(q)))
        return dq
    _attn_profile(10.0 * B * N * Nk * C, lambda: call('cmda_attention_bwd', ptr(q), ptr(kv), ptr(do), ptr(dq), ptr(dkv32), ptr(dkv16),
                                                      ptr(stats), c_i32(B), c_i32(N), c_i32(Nk), c_i32(heads), c_i32(C), c_f32(scale),
                                                      dtype_tag(q), stream_of(q)))
    return dq


def dwconv_fwd(x, w, bias, B, H, W, C, dil=1, act=None, colstats=None):
    """colstats=(ws, images_per_group): the BatchNorm statistics of y on the way (dilated walk, no activation: cmda_dwconv3x3_fwd_stats)"""
    check_dev(x, w, bias)
    y = torch.empty_like(x)
    if colstats is not None:
        assert act is None and dil >= 2
        check_dev(colstats[0])
        call('cmda_dwconv3x3_fwd_stats', ptr(x), ptr(w), ptr(bias), ptr(y), c_i32(B), c_i32(H), c_i32(W), c_i32(C), c_i32(dil),
             ptr(colstats[0]), c_i32(colstats[1]), dtype_tag(x), stream_of(x))
        return y
    call('cmda_dwconv3x3_fwd', ptr(x), ptr(w), ptr(bias), ptr(y), c_i32(B), c_i32(H), c_i32(W), c_i32(C), c_i32(dil),
         c_i32(ACT[act]), dtype_tag(x), stream_of(x))
    return y


def dwconv_gelu_bwd_prep(x, w, bias, da, B, H, W, C, dil=1):
    check_dev(x, w, bias, da)
    dz = torch.empty_like(x)
    call('cmda_dwconv3x3_gelu_bwd_prep', ptr(x), ptr(w), ptr(bias), ptr(da), ptr(dz), c_i32(B), c_i32(H), c_i32(W),
         c_i32(C), c_i32(dil), dtype_tag(x), stream_of(x))
    return dz


def dwconv_gelu_bwd_fused(x, w, bias, da, dw, dbias, B, H, W, C, dil=1):
    """dz = da * gelu'(conv(x) + bias) and the depthwise weight / bias gradients (accumulated) in one pass; returns dz"""
    check_dev(x, w, bias, da, dw, dbias)
    dz = torch.empty_like(x)
    call('cmda_dwconv3x3_gelu_bwd_fused', ptr(x), ptr(w), ptr(bias), ptr(da), ptr(dz), ptr(dw), ptr(dbias), c_i32(B), c_i32(H),
         c_i32(W), c_i32(C), c_i32(dil), dtype_tag(x), stream_of(x))
    return dz


def dwconv_bwd_data(dy, w, B, H, W, C, dil=1, out=None, accumulate=False):
    check_dev(dy, w, out)
    dx = torch.empty_like(dy) if out is None else out
    call('cmda_dwconv3x3_bwd_data', ptr(dy), ptr(w), ptr(dx), c_i32(B), c_i32(H), c_i32(W), c_i32(C), c_i32(dil),
         c_i32(int(accumulate)), dtype_tag(dy), stream_of(dy))
    return dx


def dwconv_bwd_weight(dz, x, dw, dbias, B, H, W, C, dil=1):
    check_dev(dz, x, dw, dbias)
    call('cmda_dwconv3x3_bwd_weight', ptr(dz), ptr(x), ptr(dw), ptr(dbias), c_i32(B), c_i32(H), c_i32(W), c_i32(C),
         c_i32(dil), dtype_tag(x), stream_of(x))


def bilinear_fwd(x, y, B, IH, IW, OH, OW, C, ldy=None, coff=0):
    check_dev(x, y)
    call('cmda_bilinear_fwd', ptr(x), ptr(y), c_i32(B), c_i32(IH), c_i32(IW), c_i32(OH), c_i32(OW), c_i32(C),
         c_i32(C if ldy is None else ldy), c_i32(coff), dtype_tag(x), stream_of(x))
    return y


def bilinear_bwd(dy, dx, B, IH, IW, OH, OW, C, ldy=None, coff=0):
    check_dev(dy, dx)
    call('cmda_bilinear_bwd', ptr(dy), ptr(dx), c_i32(B), c_i32(IH), c_i32(IW), c_i32(OH), c_i32(OW), c_i32(C),
         c_i32(C if ldy is None else ldy), c_i32(coff), dtype_tag(dy), stream_of(dy))
    return dx


BN_FUSED_STATS = os.environ.get('CMDA_BN_FUSED_STATS', '1') != '0'   # statistics of conv -> BN / IN pairs in the GEMM epilogue (A/B switch)
def bn_stats_ws(device, groups, C):
    """the persistent per-lane ZERO workspace a GEMM epilogue accumulates BatchNorm statistics into (gemm(colstats=...));
    bn_train_fwd / bn_train_fwd2 with stats_ws hand it back zeroed.  None where the fused statistics are switched off, and inside a
    capture for a lane nobody pre-allocated for (the separate statistics pass)."""
    if not BN_FUSED_STATS:
        return None
    need = groups * int(L.lib().cmda_bn_ws_floats(C))
    ws = D.workspace('bn', device, need, make_in_capture=False)
    return None if ws is None else ws[:need]


def colstats_ok(rows_per_group, N):
    """may the convolution in front of a BatchNorm / InstanceNorm over groups of `rows_per_group` rows and N channels take the
    statistics in its epilogue (cmda_gemm_params_t.colstats: whole 256-row tiles per group, 16-byte column quads)"""
    return BN_FUSED_STATS and rows_per_group > 0 and rows_per_group % 256 == 0 and N % 4 == 0


def bn_train_fwd(x, gamma, beta, y, running_mean, running_var, M, C, eps, momentum, relu, ldy=None, coff=0, groups=1, order=None,
                 stats_ws=None):
    """M = rows PER GROUP; x / y hold `groups` consecutive blocks of M rows (own statistics each); returns mean, rstd [groups, C].
    stats_ws: the workspace the producing GEMM's epilogue filled (gemm(colstats=(ws, M))): no statistics pass over x"""
    check_dev(x, gamma, beta, y, running_mean, running_var, stats_ws)
    mean = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    ws = stats_ws if stats_ws is not None else torch.empty(groups * L.lib().cmda_bn_ws_floats(C), dtype=torch.float32, device=x.device)
    order_c = (ctypes.c_int * groups)(*order) if order is not None else None
    call('cmda_bn_train_fwd', ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(running_mean),
         ptr(running_var), ptr(ws), c_i64(M), c_i32(C), c_f32(eps), c_f32(momentum), c_i32(int(relu)),
         c_i32(C if ldy is None else ldy), c_i32(coff), c_i32(groups), order_c, c_i32(int(stats_ws is not None)), dtype_tag(x), stream_of(x))
    return mean, rstd


def bn_train_fwd2(x, gamma, beta, y, M, C, eps, relu, groups=1, res32=None, y2=None, ldy=None, coff=0, stats_ws=None):
    """cmda_bn_train_fwd2: x and y of independent storage types, no running statistics; res32 (fp32 [groups*M, C]) is added after
    the normalisation, y2 (bf16 [groups*M, C]) receives a copy of the result.  Returns mean, rstd [groups, C].  stats_ws: bn_train_fwd"""
    check_dev(x, gamma, beta, y, res32, y2, stats_ws)
    assert res32 is None or res32.dtype == torch.float32
    assert y2 is None or y2.dtype == torch.bfloat16
    mean = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    ws = stats_ws if stats_ws is not None else torch.empty(groups * L.lib().cmda_bn_ws_floats(C), dtype=torch.float32, device=x.device)
    call('cmda_bn_train_fwd2', ptr(x), dtype_tag(x), ptr(gamma), ptr(beta), ptr(y), dtype_tag(y), ptr(mean), ptr(rstd), None, None,
         ptr(ws), c_i64(M), c_i32(C), c_f32(eps), c_f32(0.0), c_i32(int(relu)), c_i32(C if ldy is None else ldy), c_i32(coff),
         c_i32(groups), None, ptr(res32), ptr(y2), c_i32(int(stats_ws is not None)), stream_of(x))
    return mean, rstd


def bn_apply(x, mean, rstd, gamma, beta, y, M, C, relu, ldy=None, coff=0):
    check_dev(x, mean, rstd, gamma, beta, y)
    call('cmda_bn_apply', ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(y), c_i64(M), c_i32(C),
         c_i32(int(relu)), c_i32(C if ldy is None else ldy), c_i32(coff), dtype_tag(x), stream_of(x))


def bn_train_bwd(dy, x, mean, rstd, gamma, beta, dgamma, dbeta, M, C, relu, lddy=None, coff=0, groups=1):
    check_dev(dy, x, mean, rstd, gamma, beta, dgamma, dbeta)
    dx = torch.empty_like(x)
    ws = torch.empty(groups * L.lib().cmda_bn_ws_floats(C), dtype=torch.float32, device=x.device)
    call('cmda_bn_train_bwd', ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), ptr(dgamma),
         ptr(dbeta), ptr(ws), c_i64(M), c_i32(C), c_i32(int(relu)), c_i32(C if lddy is None else lddy), c_i32(coff),
         c_i32(groups), dtype_tag(x), stream_of(x))
    return dx


def ce_upsample_fwd(logits, label, weight, H, W, ignore_index=255, acc=None):
    """logits fp32 NHWC [B,h,w,nc]; returns (acc[2] = (sum w*nll, #correct), lse[B,H,W]).  acc: optional ZEROED fp32 [2] to
    accumulate into (a slice of one buffer shared by the loss terms of a pass)"""
    check_dev(logits, label, weight, acc)
    B, h, w, nc = logits.shape
    lse = torch.empty(B, H, W, dtype=torch.float32, device=logits.device)
    if acc is None:
        acc = torch.zeros(2, dtype=torch.float32, device=logits.device)
    call('cmda_ce_upsample_fwd', ptr(logits), ptr(label), ptr(weight), ptr(lse), ptr(acc), c_i32(B), c_i32(h), c_i32(w),
         c_i32(H), c_i32(W), c_i32(nc), c_i32(ignore_index), stream_of(logits))
    return acc, lse


def ce_upsample_bwd(logits, label, weight, lse, gscale, gscale_mul, H, W, ignore_index=255, out=None):
    check_dev(logits, label, weight, lse, gscale, out)
    B, h, w, nc = logits.shape
    dl = torch.empty_like(logits) if out is None else out
    call('cmda_ce_upsample_bwd', ptr(logits), ptr(label), ptr(weight), ptr(lse), ptr(gscale), c_f32(gscale_mul), ptr(dl),
         c_i32(B), c_i32(h), c_i32(w), c_i32(H), c_i32(W), c_i32(nc), c_i32(ignore_index), stream_of(logits))
    return dl


_FD_TICKETS = {}


def _fd_ticket(device, slot):
    """the arrival ticket of a feature-distance launch (zero between launches, see include/cmda_hip.h): one persistent int32 per
    device and entry point, allocated before any capture sees it"""
    key = (str(device), slot)
    t = _FD_TICKETS.get(key)
    if t is None:
        t = _FD_TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def fdist_label_mask(label, h, w, classes, min_ratio, num_classes=19, ignore_index=255):
    """downscale_label_ratio (utils/utils.py:18-39) + the class mask of calc_feat_dist (dacs.py:338-345) on the device.  label:
    int64 [B,H,W] or [B,1,H,W] with H = h*s, W = w*s.  Returns (rescaled int64 [B,h,w], mask uint8 [B,h,w], count int32 [1]) --
    the count stays on the device."""
    check_dev(label)
    B, H, W = label.shape[0], label.shape[-2], label.shape[-1]
    bits = 0
    for c in classes:
        if not 0 <= int(c) < 32:
            raise L.CmdaError(f'feature-distance class {c} outside 0..31')
        bits |= 1 << int(c)
    dev = label.device
    rescaled = torch.empty(B, h, w, dtype=torch.int64, device=dev)
    mask = torch.empty(B, h, w, dtype=torch.uint8, device=dev)
    rows = torch.empty(B * h, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    call('cmda_fdist_label_mask', ptr(label), c_i32(B), c_i32(H), c_i32(W), c_i32(h), c_i32(w), c_i32(num_classes),
         c_i32(ignore_index), c_f32(min_ratio), ctypes.c_uint32(bits), ptr(rescaled), ptr(mask), ptr(rows), ptr(count),
         ptr(_fd_ticket(dev, 0)), stream_of(label))
    return rescaled, mask, count


def fdist_fwd_bwd(fs, ft, lam, mask=None, count=None, gscale=None, grad=None):
    """masked_feat_dist (dacs.py:318-326) times lambda, and its gradient with respect to `fs` ADDED into `grad`.  fs / ft: student /
    frozen-encoder rows [R, C] in the compute dtype; mask: uint8 [R] (None: every row) with its device count int32 [1]; gscale:
    fp32 [1] device scale of the gradient (None: 1); grad: [R, C] rows (row stride grad.stride(0)) of fs's dtype (or fp32 under
    bf16 rows), or None.
    Returns (loss fp32 [1], per-row norms fp32 [R])."""
    check_dev(fs, ft, mask, count, gscale)
    R, C = fs.shape
    assert ft.shape == fs.shape and ft.dtype == fs.dtype
    assert (mask is None) == (count is None)
    if grad is not None:
        if L.emulated() and grad.is_cuda or (not L.emulated() and not grad.is_cuda):
            raise L.CmdaError('gradient block on the wrong device')
        assert grad.shape == fs.shape and grad.stride(1) == 1
    loss = torch.empty(1, dtype=torch.float32, device=fs.device)
    norms = torch.empty(R, dtype=torch.float32, device=fs.device)
    call('cmda_fdist_fwd_bwd', ptr(fs), ptr(ft), ptr(mask), ptr(count), c_i32(R), c_i32(C),
         c_i64(grad.stride(0) if grad is not None else C), c_f32(lam), ptr(gscale), ptr(grad), ptr(norms), ptr(loss),
         ptr(_fd_ticket(fs.device, 1)), c_i32(dtype_tag(fs)), c_i32(dtype_tag(grad) if grad is not None else dtype_tag(fs)),
         stream_of(fs))
    return loss, norms


def feat_consis(levels_a, levels_b, lam, gscale=None, grads=None, want_loss=True):
    """The feature-consistency loss of the `isr_no_fusion` route (encoder_decoder.py:833-848): sum over the levels of
    lam * F.mse_loss(a_l, b_l.detach()), and its gradient with respect to a_l ADDED into grads[l] -- every level in ONE launch.
    levels_a / levels_b: 1 to 4 pairs of rows [R_l, C_l] in the compute dtype (unit column stride, any row stride: blocks of wider
    buffers are fine); gscale: fp32 [1] device scale of the gradient (None: 1); grads: None (loss only), or one entry per level, each
    None or an [R_l, C_l] block (row stride grads[l].stride(0)) of the features' dtype (or fp32 under bf16 features; one dtype for
    all).  want_loss=False: gradient only.
    Returns (loss fp32 [1], level_loss fp32 [n_levels]), or (None, None) when want_loss is False."""
    n = len(levels_a)
    assert n == len(levels_b) and (grads is None or len(grads) == n)
    grads = list(grads) if grads is not None else [None] * n
    given = [g for g in grads if g is not None]
    if n < 1 or n > 4:
        raise L.CmdaError(f'feat_consis: {n} levels (1 to 4)')
    if not want_loss and not given:
        raise L.CmdaError('feat_consis: neither the loss nor a gradient block is asked for')
    first = levels_a[0]
    dev = first.device
    for t in (gscale, *levels_a, *levels_b, *given):
        if t is None:
            continue
        if L.emulated() == t.is_cuda:
            raise L.CmdaError('feat_consis: tensor on the wrong device')
    if gscale is not None:
        check_dev(gscale)
    arr = (L.Level9 * n)()
    for d, a, b, g in zip(arr, levels_a, levels_b, grads):
        assert a.dim() == 2 and a.shape == b.shape and a.dtype == b.dtype == first.dtype and a.stride(1) == 1 and b.stride(1) == 1
        d.a, d.b, d.R, d.C, d.lda, d.ldb = a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], a.stride(0), b.stride(0)
        if g is not None:
            assert g.shape == a.shape and g.stride(1) == 1 and g.dtype == given[0].dtype
            d.grad, d.ldg = g.data_ptr(), g.stride(0)
    ftag = dtype_tag(first)
    loss = level_loss = ticket = ws = None
    if want_loss:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        level_loss = torch.empty(n, dtype=torch.float32, device=dev)
        ticket = _fd_ticket(dev, 2)
        nws = int(L.lib().cmdax9_ws_floats(arr, n, ftag))
        if nws < 0:
            raise L.CmdaError('cmdax9_ws_floats failed: bad shape')
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
    call('cmdax9_feat_consis', arr, c_i32(n), c_f32(lam), ptr(gscale), ptr(loss), ptr(level_loss), ptr(ticket), ptr(ws),
         c_i32(ftag), c_i32(dtype_tag(given[0]) if given else ftag), stream_of(first))
    return loss, level_loss


def pseudo_label(logits, H, W, thr, want_prob=True):
    check_dev(logits)
    B, h, w, nc = logits.shape
    label = torch.empty(B, H, W, dtype=torch.int64, device=logits.device)
    prob = torch.empty(B, H, W, dtype=torch.float32, device=logits.device) if want_prob else None
    count = torch.zeros(1, dtype=torch.int32, device=logits.device)
    call('cmda_pseudo_label', ptr(logits), ptr(label), ptr(prob), ptr(count), c_i32(B), c_i32(h), c_i32(w), c_i32(H),
         c_i32(W), c_i32(nc), c_f32(thr), stream_of(logits))
    return label, prob, count


def pseudo_weight(count, B, H, W, top=0, bottom=0):
    check_dev(count)
    wgt = torch.empty(B, H, W, dtype=torch.float32, device=count.device)
    call('cmda_pseudo_weight', ptr(count), ptr(wgt), c_i32(B), c_i32(H), c_i32(W), c_i32(top), c_i32(bottom),
         stream_of(count))
    return wgt


def sample_scale(x, scale, B, C, per_channel=False, out=None):
    """x viewed as [B, HW*C]; scale fp32 [B] or [B,C]."""
    check_dev(x, scale, out)
    out = torch.empty_like(x) if out is None else out
    call('cmda_sample_scale', ptr(x), ptr(scale), ptr(out), c_i32(B), c_i64(x.numel() // B), c_i32(C),
         c_i32(int(per_channel)), dtype_tag(x), stream_of(x))
    return out


def upsample_logits_nchw(logits, H, W):
    """fp32 NHWC [B,h,w,nc] -> fp32 NCHW [B,nc,H,W] (bilinear, align_corners=False)."""
    check_dev(logits)
    B, h, w, nc = logits.shape
    out = torch.empty(B, nc, H, W, dtype=torch.float32, device=logits.device)
    call('cmda_upsample_logits_nchw', ptr(logits), ptr(out), c_i32(B), c_i32(h), c_i32(w), c_i32(H), c_i32(W), c_i32(nc),
         stream_of(logits))
    return out


FLIP_NONE, FLIP_HORIZONTAL, FLIP_VERTICAL = 0, 1, 2


def _check_conf(conf, nc):
    if conf.dtype != torch.int64 or conf.numel() != (nc + 1) * nc:
        raise L.CmdaError(f'conf must be int64 with ({nc} + 1) * {nc} cells, got {conf.dtype} {tuple(conf.shape)}')


def seg_predict(logits, H, W, out_hw=None, flip=0, gt=None, conf=None, ignore_index=255, out=None):
    """The evaluation tail in one launch: fp32 NHWC logits [B,h,w,nc] -> uint8 labels [B,OH,OW] = first arg-max of the logits
    up-sampled to H x W (the network input), resized to out_hw = (OH, OW) when that differs, flipped back (flip: 0 none,
    1 horizontal, 2 vertical).  With `gt` (uint8 / int64 [B,OH,OW], un-flipped frame) and `conf` (int64 [(nc+1), nc]) the
    confusion counters are updated in the same launch: conf[gt or nc][label] += 1 where gt != ignore_index; accumulated, never
    cleared here.  `out`: an existing uint8 [B,OH,OW] tensor to write into."""
    check_dev(logits, gt, conf, out)
    if logits.dtype != torch.float32 or logits.dim() != 4:
        raise L.CmdaError('seg_predict expects fp32 NHWC logits [B,h,w,nc]')
    B, h, w, nc = logits.shape
    OH, OW = (int(out_hw[0]), int(out_hw[1])) if out_hw is not None else (int(H), int(W))
    if out is None:
        out = torch.empty(B, max(OH, 0), max(OW, 0), dtype=torch.uint8, device=logits.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, OH, OW):
        raise L.CmdaError(f'seg_predict: out must be uint8 {(B, OH, OW)}')
    gt_tag = 0
    if gt is not None:
        gt_tag = L.label_tag(gt)
        if gt.numel() != B * OH * OW:
            raise L.CmdaError(f'seg_predict: gt has {gt.numel()} labels for {B} x {OH} x {OW} pixels')
    if conf is not None and 1 <= nc <= 32:
        _check_conf(conf, nc)
    call('cmdax_seg_predict', ptr(logits), ptr(out), ptr(gt), c_i32(gt_tag), ptr(conf), c_i32(B), c_i32(h), c_i32(w), c_i32(H),
         c_i32(W), c_i32(OH), c_i32(OW), c_i32(nc), c_i32(int(flip)), c_i32(ignore_index), stream_of(logits))
    return out


def confusion_update(pred, gt, conf, num_classes, ignore_index=255):
    """conf (int64 [(nc+1), nc], accumulated) += the confusion counters of the label maps pred / gt (uint8 or int64, the same
    number of pixels): row = gt (row nc: out of range but not ignored), column = pred; pixels with gt == ignore_index and
    predictions outside [0, nc) are not counted."""
    check_dev(pred, gt, conf)
    if pred.numel() != gt.numel():
        raise L.CmdaError(f'confusion_update: {pred.numel()} predictions for {gt.numel()} labels')
    if 1 <= num_classes <= 32:
        _check_conf(conf, num_classes)
    call('cmdax_confusion_update', ptr(pred), c_i32(L.label_tag(pred)), ptr(gt), c_i32(L.label_tag(gt)), ptr(conf),
         c_i64(pred.numel()), c_i32(num_classes), c_i32(ignore_index), stream_of(conf))
    return conf


SCORES_LABELS, SCORES_PROBS = 0, 1   # cmdax2_seg_scores `mode`


def slide_windows(H, W, crop, stride):
    """The reference's sliding-window grid (encoder_decoder.py:183-196): the list of (y1, x1, y2, x2), rows of windows outermost;
    a window the border would cut is shifted back, so every window has the size min(crop, image)."""
    (H, W), (ch, cw), (sh, sw) = (int(H), int(W)), (int(crop[0]), int(crop[1])), (int(stride[0]), int(stride[1]))
    if min(H, W, ch, cw, sh, sw) < 1:
        raise L.CmdaError(f'slide_windows: sizes, crop and stride must be at least 1, got {(H, W)}, {(ch, cw)}, {(sh, sw)}')
    out = []
    for i in range(max(H - ch + sh - 1, 0) // sh + 1):
        for j in range(max(W - cw + sw - 1, 0) // sw + 1):
            y2, x2 = min(i * sh + ch, H), min(j * sw + cw, W)
            out.append((max(y2 - ch, 0), max(x2 - cw, 0), y2, x2))
    return out


def _window_args(name, logits, H, W, crop, stride, out_hw):
    """shared argument checks of the two window ops: (K, B, hl, wl, nc, OH, OW, the six grid scalars as c_i32)"""
    if logits.dtype != torch.float32 or logits.dim() != 5:
        raise L.CmdaError(f'{name} expects fp32 NHWC logits of all windows [K,B,hl,wl,nc]')
    K, B, hl, wl, nc = logits.shape
    (ch, cw), (sh, sw) = (int(crop[0]), int(crop[1])), (int(stride[0]), int(stride[1]))
    if min(int(H), int(W), ch, cw, sh, sw) >= 1:   # (anything below 1 is the kernel library's refusal)
        want = (max(H - ch + sh - 1, 0) // sh + 1) * (max(W - cw + sw - 1, 0) // sw + 1)
        if K != want:
            raise L.CmdaError(f'{name}: {K} windows given, the grid of crop {(ch, cw)} / stride {(sh, sw)} on {(H, W)} has {want}')
    OH, OW = (int(out_hw[0]), int(out_hw[1])) if out_hw is not None else (int(H), int(W))
    grid = [c_i32(int(v)) for v in (H, W, ch, cw, sh, sw)]
    return K, B, hl, wl, nc, OH, OW, grid


def seg_predict_windows(logits, H, W, crop, stride, out_hw=None, flip=0, gt=None, conf=None, ignore_index=255, out=None):
    """The evaluation tail of test_cfg.mode 'slide' in one launch: fp32 NHWC logits of all windows [K,B,hl,wl,nc] (window order of
    `slide_windows(H, W, crop, stride)`) -> uint8 labels [B,OH,OW] = first arg-max of (the sum over the covering windows of the
    logits up-sampled to the window size) / (their number), resized to out_hw = (OH, OW) when that differs from (H, W), flipped
    back.  `flip`, `gt`, `conf`, `ignore_index`, `out`: as `seg_predict`, whose result this is when one window covers the image."""
    check_dev(logits, gt, conf, out)
    K, B, hl, wl, nc, OH, OW, grid = _window_args('seg_predict_windows', logits, H, W, crop, stride, out_hw)
    if out is None:
        out = torch.empty(B, max(OH, 0), max(OW, 0), dtype=torch.uint8, device=logits.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, OH, OW):
        raise L.CmdaError(f'seg_predict_windows: out must be uint8 {(B, OH, OW)}')
    gt_tag = 0
    if gt is not None:
        gt_tag = L.label_tag(gt)
        if gt.numel() != B * OH * OW:
            raise L.CmdaError(f'seg_predict_windows: gt has {gt.numel()} labels for {B} x {OH} x {OW} pixels')
    if conf is not None and 1 <= nc <= 32:
        _check_conf(conf, nc)
    call('cmdax2_seg_scores', ptr(logits), c_i32(SCORES_LABELS), ptr(out), None, c_i32(0), ptr(gt), c_i32(gt_tag), ptr(conf), c_i32(B),
         c_i32(hl), c_i32(wl), *grid, c_i32(OH), c_i32(OW), c_i32(nc), c_i32(int(flip)), c_i32(ignore_index), stream_of(logits))
    return out


def seg_prob_accumulate(logits, H, W, crop, stride, out_hw, flip, acc, accumulate):
    """One view of the multi-view test in one launch: acc (fp32 NCHW [B,nc,OH,OW]) = (acc if accumulate else 0) + soft-max over
    the classes of the view's scores at out_hw = (OH, OW), flipped back -- scores as in `seg_predict_windows` (test_cfg.mode
    'whole' is the grid of one window: crop = stride = (H, W) and logits [1,B,hl,wl,nc])."""
    check_dev(logits, acc)
    K, B, hl, wl, nc, OH, OW, grid = _window_args('seg_prob_accumulate', logits, H, W, crop, stride, out_hw)
    if acc.dtype != torch.float32 or tuple(acc.shape) != (B, nc, OH, OW):
        raise L.CmdaError(f'seg_prob_accumulate: acc must be fp32 {(B, nc, OH, OW)}, got {acc.dtype} {tuple(acc.shape)}')
    call('cmdax2_seg_scores', ptr(logits), c_i32(SCORES_PROBS), None, ptr(acc), c_i32(int(bool(accumulate))), None, c_i32(0), None,
         c_i32(B), c_i32(hl), c_i32(wl), *grid, c_i32(OH), c_i32(OW), c_i32(nc), c_i32(int(flip)), c_i32(255), stream_of(logits))
    return acc


def prob_predict(acc, n, gt=None, conf=None, ignore_index=255, out=None):
    """The end of the multi-view test in one launch: summed probabilities of n views (fp32 NCHW [B,nc,OH,OW]) -> uint8 labels
    [B,OH,OW] = first arg-max of acc / n; `gt`, `conf`, `ignore_index`, `out`: as `seg_predict`."""
    check_dev(acc, gt, conf, out)
    if acc.dtype != torch.float32 or acc.dim() != 4:
        raise L.CmdaError('prob_predict expects fp32 NCHW probabilities [B,nc,OH,OW]')
    B, nc, OH, OW = acc.shape
    if out is None:
        out = torch.empty(B, OH, OW, dtype=torch.uint8, device=acc.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, OH, OW):
        raise L.CmdaError(f'prob_predict: out must be uint8 {(B, OH, OW)}')
    gt_tag = 0
    if gt is not None:
        gt_tag = L.label_tag(gt)
        if gt.numel() != B * OH * OW:
            raise L.CmdaError(f'prob_predict: gt has {gt.numel()} labels for {B} x {OH} x {OW} pixels')
    if conf is not None and 1 <= nc <= 32:
        _check_conf(conf, nc)
    call('cmdax2_prob_predict', ptr(acc), ptr(out), ptr(gt), c_i32(gt_tag), ptr(conf), c_i32(B), c_i32(OH), c_i32(OW), c_i32(nc),
         c_i32(int(n)), c_i32(ignore_index), stream_of(acc))
    return out


def copy2d(src, dst, rows, cols, src_ld, dst_ld, src_off=0, dst_off=0):
    check_dev(src, dst)
    es = _ESIZE[src.dtype]
    call('cmda_copy2d', L.c_vp(src.data_ptr() + src_off * es), L.c_vp(dst.data_ptr() + dst_off * es), c_i64(rows),
         c_i32(cols), c_i64(src_ld), c_i64(dst_ld), dtype_tag(src), stream_of(src))
    return dst


_IMG_MEAN = (ctypes.c_float * 3)(123.675, 116.28, 103.53)
_IMG_STD = (ctypes.c_float * 3)(58.395, 57.12, 57.375)
_ISR_DIRS = {'rightdown': ((0, -1), (-1, 0)), 'rightup': ((0, -1), (1, 0)), 'leftdown': ((0, 1), (-1, 0)),
             'leftup': ((0, 1), (1, 0)), 'all': ((1, 0), (0, 1), (-1, 0), (0, -1))}


_ISR_LUT = {}


def isr_lut(val_range, device):
    """float32 log-intensity of the 256 gray levels, computed exactly as datasets/utils.py:get_ic does (numpy fp32); cached per
    (value range, device) -- the table is a constant of the configuration."""
    key = (float(val_range[0]), float(val_range[1]), str(device))
    lut = _ISR_LUT.get(key)
    if lut is None:
        g = np.arange(256, dtype=np.float32)
        lut = torch.from_numpy(np.log(g / 255 * (val_range[1] - val_range[0]) + val_range[0]).astype(np.float32)).to(device)
        _ISR_LUT[key] = lut
    return lut


def isr_dirs(shift_direction, shift_pixel):
    """host list of (dy, dx) shifts of get_image_change_from_pil (datasets/utils.py:108-152) for a direction name"""
    return [(dy * shift_pixel, dx * shift_pixel) for dy, dx in _ISR_DIRS[shift_direction]]


def isr_gray(img):
    """normalised NCHW fp32 image [B,3,H,W] -> PIL-exact 'L' uint8 [B,H,W]"""
    check_dev(img)
    B, _, H, W = img.shape
    gray = torch.empty(B, H, W, dtype=torch.uint8, device=img.device)
    call('cmda_isr_gray', ptr(img), ptr(gray), c_i32(B), c_i32(H), c_i32(W), _IMG_MEAN, _IMG_STD, stream_of(img))
    return gray


def isr_from_gray(gray, val_range, threshold, clip_range, shift_pixel, shift_direction, dirs_dev=None):
    """get_image_change_from_pil after the gray conversion -> fp32 NCHW [B,3,H,W] in [-1,1].  `dirs_dev`: optional DEVICE
    int32 [ndir,2] holding the (dy,dx) shifts (then `shift_direction` only gives ndir); lets a captured launch sequence pick
    the direction per replay."""
    check_dev(gray, dirs_dev)
    B, H, W = gray.shape
    span = np.log(val_range[1]) - np.log(val_range[0])
    dirs = isr_dirs(shift_direction, shift_pixel)
    dirs_t = dirs_dev if dirs_dev is not None else torch.tensor(dirs, dtype=torch.int32).to(gray.device)
    mm = torch.empty(B * len(dirs) * 4, dtype=torch.int32, device=gray.device)
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=gray.device)
    lut = isr_lut(val_range, gray.device)
    call('cmda_isr_from_gray', ptr(gray), ptr(lut), ptr(dirs_t), c_i32(len(dirs)), ptr(mm),
         ptr(out), c_i32(B), c_i32(H), c_i32(W), c_f32(float(np.float32(span * threshold))),
         c_f32(float(np.float32(span * clip_range))), stream_of(gray))
    return out


def events_to_voxel_grid(t, x, y, pol, bins, H, W):
    check_dev(t, x, y, pol)
    grid = torch.empty(bins, H, W, dtype=torch.float32, device=t.device)
    call('cmda_events_to_voxel_grid', ptr(t), ptr(x), ptr(y), ptr(pol), ptr(grid), c_i64(t.numel()), c_i32(bins), c_i32(H),
         c_i32(W), stream_of(t))
    return grid


def events_norm(events, clip_range, final_range=1.0):
    check_dev(events)
    out = torch.empty_like(events)
    ws = torch.empty(5, dtype=torch.float64, device=events.device)
    call('cmda_events_norm', ptr(events), ptr(out), ptr(ws), c_i64(events.numel()), c_f32(clip_range), c_f32(final_range),
         stream_of(events))
    return out


def jitter_params(per_sample):
    """host list of B tuples (order[4], f_b, f_c, f_s, f_h) -> CPU fp32 [B,8] (the layout cmda_color_jitter reads)"""
    return torch.tensor([[float(v) for v in order] + [fb, fc, fs, fh] for order, fb, fc, fs, fh in per_sample],
                        dtype=torch.float32)


def color_jitter_(img, prm, enable=None):
    """In place on the normalised NCHW fp32 image: kornia-0.5 ColorJitter, one (op order, factors) row of the DEVICE fp32
    tensor `prm` [B,8] per sample; `enable`: optional DEVICE int32 gate (0 = leave the image untouched)."""
    check_dev(img, prm, enable)
    B, _, H, W = img.shape
    assert prm.shape == (B, 8) and prm.dtype == torch.float32
    call('cmda_color_jitter', ptr(img), c_i32(B), c_i32(H), c_i32(W), _IMG_MEAN, _IMG_STD, ptr(prm), ptr(enable), stream_of(img))
    return img


def gaussian_taps(k, sigma, device=None):
    x = torch.arange(k, dtype=torch.float32) - k // 2
    g = torch.exp(-x * x / (2.0 * sigma * sigma))
    g = g / g.sum()
    return g if device is None else g.to(device)


def blur_kernel_size(n):
    """dacs_transforms.py:86-93: kernel size from the image extent n"""
    return int(np.floor(np.ceil(0.1 * n) - 0.5 + np.ceil(0.1 * n) % 2))


def gaussian_blur_(img, taps_x, taps_y, enable=None):
    """In place separable Gaussian blur (reflect border) of an NCHW fp32 image; taps_x / taps_y: DEVICE fp32 normalised
    Gaussians (lengths kx from W, ky from H); `enable`: optional DEVICE int32 gate."""
    check_dev(img, taps_x, taps_y, enable)
    B, C, H, W = img.shape
    tmp = torch.empty_like(img)
    call('cmda_gaussian_blur', ptr(img), ptr(tmp), ptr(taps_x), ptr(taps_y), c_i32(B * C), c_i32(H), c_i32(W),
         c_i32(taps_x.numel()), c_i32(taps_y.numel()), ptr(enable), stream_of(img))
    return img


# ---- ISR augmentations (isr_augment.hip, include/cmda_hip_ext3.h): sky mask and sensor noise ----------------------------------------
SKY_CHUNK = 8          # chunk size of the noise shuffle (dacs_transforms.py:138)
SKY_MIN_PIXELS = 10    # fewer sky pixels: sky_mask_transform returns its input (:140)
ISR_NOISE_TYPES = ('', 'noise', 'blur', 'noise+blur')
# ranges of add_noise_on_isr's draws (dacs_transforms.py:196-198; cityscapes_ic.py:85-87): |n1| < t1 keeps, |n2| < t2 adds, intensity
ISR_NOISE_RANGES = ((1.0, 1.5), (0.4, 0.6), (0.1, 0.3))


def load_noise_bank(src):
    """the sky-mask noise bank as a CPU uint8 tensor [N,H,W].  `src`: a directory, read as the reference reads it (os.listdir order,
    one image per file through PIL; `.npy` files are accepted as well), or a uint8 tensor / array [N,H,W]."""
    if isinstance(src, (str, os.PathLike)):
        imgs = []
        for name in os.listdir(src):
            path = os.path.join(src, name)
            if name.endswith('.npy'):
                a = np.load(path)
            else:
                from PIL import Image
                a = np.array(Image.open(path))
            imgs.append(torch.from_numpy(np.ascontiguousarray(a)))
        if not imgs:
            raise ValueError(f'sky_mask: no noise image in {src!r}')
        bank = torch.stack(imgs)
    else:
        bank = torch.as_tensor(src)
    if bank.dtype != torch.uint8 or bank.dim() != 3 or bank.shape[0] < 1:
        raise ValueError(f'sky_mask: the noise bank must be uint8 [N,H,W], got {bank.dtype} {tuple(bank.shape)}')
    return bank.contiguous()


def _shuffled_axis(n):
    """torch.split(chunk 8) -> randperm over the chunks -> cat (dacs_transforms.py:162-166) as the source index of every output
    index; a short last chunk moves like any other"""
    chunks = torch.split(torch.arange(n, dtype=torch.int32), SKY_CHUNK)
    order = torch.randperm(len(chunks))
    return torch.cat([chunks[int(i)] for i in order])


def draw_sky_mask(n_noise, H, W, sky_count=None):
    """The host decisions of ONE sky_mask_transform call, drawn from the torch CPU generator in the reference's order:
    randint(21, 61) (made odd), uniform_(0.1, 0.3), uniform_(0.5, 1.2), randint(0, n_noise), randperm(row chunks), randperm(column
    chunks).  With `sky_count` given and below 10 it stops after the third draw, as the reference's early return does.  Without
    `sky_count` all six are drawn always -- the kernel decides on the device whether the sample is transformed -- so the torch
    stream then differs from the reference's for samples with fewer than 10 sky pixels.
    Returns dict(k, lam, intensity, index, rows int32 [H], cols int32 [W]): rows / cols = the bank row / column per output row / column."""
    k = int(torch.randint(21, 61, size=(1,)).item())
    lam = torch.empty(size=(1,)).uniform_(0.1, 0.3).item()
    intensity = torch.empty(size=(1,)).uniform_(0.5, 1.2).item()
    if k % 2 == 0:
        k += 1
    d = dict(k=k, lam=lam, intensity=intensity, index=0, rows=None, cols=None)
    if sky_count is not None and int(sky_count) < SKY_MIN_PIXELS:
        d['rows'], d['cols'] = torch.arange(H, dtype=torch.int32), torch.arange(W, dtype=torch.int32)
        return d
    d['index'] = int(torch.randint(0, n_noise, size=(1,)).item())
    d['rows'] = _shuffled_axis(H)
    d['cols'] = _shuffled_axis(W)
    return d


def _f32_bits(values):
    return torch.tensor(values, dtype=torch.float32).view(torch.int32)


def sky_mask_params(draws):
    """list of draw_sky_mask dicts -> CPU (prm int32 [B,4], rows int32 [B,H], cols int32 [B,W]): the layout cmdax3_sky_mask reads"""
    prm = torch.empty(len(draws), 4, dtype=torch.int32)
    prm[:, 0] = torch.tensor([d['k'] for d in draws], dtype=torch.int32)
    prm[:, 1] = torch.tensor([d['index'] for d in draws], dtype=torch.int32)
    prm[:, 2] = _f32_bits([d['lam'] for d in draws])
    prm[:, 3] = _f32_bits([d['intensity'] for d in draws])
    return prm, torch.stack([d['rows'] for d in draws]), torch.stack([d['cols'] for d in draws])


def sky_mask(label, isr, bank, prm, rows, cols, enable=None, out=None, debug=False, k_host=None):
    """sky_mask_transform for a batch (three launches, no host sync).  label uint8 / int64 [B,H,W] (or [B,1,H,W]); isr fp32
    [B,C,H,W], C in {1, 3}; bank uint8 [N,H,W]; prm / rows / cols: DEVICE tensors in the layout of `sky_mask_params`; enable:
    optional DEVICE int32 [B].  A sample with fewer than 10 sky pixels, a closed gate or an invalid k comes back bit-equal to its
    input.  An all-sky sample, where the reference divides 0 by 0, takes a normalised weight of 0 (blur_w = 1) and stays finite.
    Out of place unless `out` is given (`out=isr` is allowed).  debug: also return (expansion, blur_w) fp32 [B,H,W].
    k_host: the kernel sizes as the host knows them, checked before anything is launched."""
    check_dev(label, isr, bank, prm, rows, cols, enable, out)
    B, C, H, W = isr.shape
    if isr.dtype != torch.float32 or bank.dtype != torch.uint8 or bank.dim() != 3:
        raise L.CmdaError('sky_mask: isr must be fp32 and the bank uint8 [N,H,W]')
    if label.numel() != B * H * W:
        raise L.CmdaError(f'sky_mask: label {tuple(label.shape)} does not match isr {tuple(isr.shape)}')
    assert prm.shape == (B, 4) and prm.dtype == torch.int32 and rows.shape == (B, H) and cols.shape == (B, W)
    assert rows.dtype == torch.int32 and cols.dtype == torch.int32 and (enable is None or enable.dtype == torch.int32)
    if out is None:
        out = torch.empty_like(isr)
    dbg_e = torch.empty(B, H, W, dtype=torch.float32, device=isr.device) if debug else None
    dbg_w = torch.empty(B, H, W, dtype=torch.float32, device=isr.device) if debug else None
    ws = torch.empty(max(1, L.lib().cmdax3_sky_mask_ws_bytes(B, H, W)), dtype=torch.uint8, device=isr.device)
    kc = (ctypes.c_int * B)(*[int(v) for v in k_host]) if k_host is not None else None
    call('cmdax3_sky_mask', ptr(label), c_i32(L.label_tag(label)), ptr(isr), ptr(bank), ptr(prm), ptr(rows), ptr(cols), ptr(enable),
         ptr(out), ptr(dbg_e), ptr(dbg_w), ptr(ws), kc, c_i32(B), c_i32(C), c_i32(H), c_i32(W), c_i32(bank.shape[0]),
         c_i32(bank.shape[1]), c_i32(bank.shape[2]), stream_of(isr))
    return (out, dbg_e, dbg_w) if debug else out


def draw_isr_noise(mode, source='torch'):
    """The host decisions of ONE add_noise_on_isr call -> (blur gate, t1, t2, intensity).  source 'torch' (DACS,
    dacs_transforms.py:186-211): torch.rand(1) coin when `mode` has 'blur', then three uniform_ draws when it has 'noise'.
    source 'random' (the loader, cityscapes_ic.py:244-257): the same coin, then random.uniform x 3.  The reference's randn_like
    fields are NOT drawn here: the kernel generates its own (`isr_noise`), which consumes nothing from torch's generators."""
    import random
    blur, t = 0, [0.0, 0.0, 0.0]
    if 'blur' in mode:
        blur = int(bool(torch.rand(1) < 0.5))
    if 'noise' in mode:
        for i, rng in enumerate(ISR_NOISE_RANGES):
            t[i] = random.uniform(*rng) if source == 'random' else torch.empty(size=(1,)).uniform_(*rng).item()
    return (blur, t[0], t[1], t[2])


def isr_noise_params(draws):
    """list of draw_isr_noise tuples -> CPU int32 [B,4]: the layout cmdax3_isr_noise reads"""
    prm = torch.empty(len(draws), 4, dtype=torch.int32)
    prm[:, 0] = torch.tensor([d[0] for d in draws], dtype=torch.int32)
    for j in (1, 2, 3):
        prm[:, j] = _f32_bits([d[j] for d in draws])
    return prm


def _offset_args(offset, offset_dev):
    if offset_dev is not None:
        assert offset_dev.dtype == torch.int64 and offset_dev.numel() == 1
    return c_i64(int(offset)), ptr(offset_dev)


def randn_fields(B, H, W, seed, offset=0, offset_dev=None, device=None):
    """fp32 [3,B,H,W]: the three standard-normal fields `isr_noise` generates for (seed, offset [+ the DEVICE int64 offset_dev])
    -- Philox4x32-10 + Box-Muller, counter (offset, sample, field, pixel); no generator of torch is touched"""
    check_dev(offset_dev)
    dev = offset_dev.device if offset_dev is not None else torch.device(device if device is not None else ('cpu' if L.emulated() else 'cuda'))
    out = torch.empty(3, B, H, W, dtype=torch.float32, device=dev)
    off, offd = _offset_args(offset, offset_dev)
    call('cmdax3_randn_fields', ptr(out), c_i32(B), c_i32(H), c_i32(W), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), off, offd,
         stream_of(out))
    return out


def isr_noise(isr, prm, mode, fields=None, seed=0, offset=0, offset_dev=None, enable=None, out=None):
    """add_noise_on_isr on channel 0 of the fp32 NCHW [B,C,H,W] ISR, the result on all C channels (one launch).  prm: DEVICE int32
    [B,4] (`isr_noise_params`); mode in ISR_NOISE_TYPES; fields: optional fp32 [3,B,H,W] (n1, n2, n3) -- without them the kernel
    generates `randn_fields(seed, offset)` in registers, bit-equal to passing those; enable: optional DEVICE int32 [B]."""
    check_dev(isr, prm, fields, offset_dev, enable, out)
    if mode not in ISR_NOISE_TYPES:
        raise ValueError(f'isr_noise: mode {mode!r} not in {ISR_NOISE_TYPES}')
    B, C, H, W = isr.shape
    assert isr.dtype == torch.float32 and prm.shape == (B, 4) and prm.dtype == torch.int32
    assert enable is None or enable.dtype == torch.int32
    if fields is not None:
        assert fields.shape == (3, B, H, W) and fields.dtype == torch.float32
    if out is None:
        out = torch.empty_like(isr)
    n = [None] * 3 if fields is None else [fields[0], fields[1], fields[2]]
    off, offd = _offset_args(offset, offset_dev)
    call('cmdax3_isr_noise', ptr(isr), ptr(out), ptr(n[0]), ptr(n[1]), ptr(n[2]), ptr(prm), ptr(enable), c_i32(B), c_i32(C), c_i32(H),
         c_i32(W), c_i32(int('blur' in mode)), c_i32(int('noise' in mode)), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), off, offd,
         stream_of(isr))
    return out


# ---- multi-parameter ISR and cow mask (isr_multi.hip, cow_mask.hip, include/cmda_hip_ext4.h) ----------------------------------------
ISR_MULTI_ROW = 12   # int32 words per parameter row (CMDAX4_ISR_ROW)
_ROOT_2, _ROOT_2_PI = 1.4142135623730951, 2.5066282746310002   # datasets/utils.py's constants (math.sqrt)


def _isr_multi_rows(parms):
    """list of dicts (the reference's spelling: val_range, _threshold, _clip_range, shift_pixel) or of (threshold, clip_range,
    shift_pixel) tuples -> (val_range or None, [(threshold, clip_range, shift_pixel)])"""
    ranges, rows = set(), []
    for p in parms:
        if isinstance(p, dict):
            ranges.add((float(p['val_range'][0]), float(p['val_range'][1])))
            rows.append((p['_threshold'], p['_clip_range'], int(p['shift_pixel'])))
        else:
            rows.append((p[0], p[1], int(p[2])))
    assert len(ranges) <= 1, f'isr_multi: one value range per call, got {sorted(ranges)}'
    return (ranges.pop() if ranges else None), rows


def isr_multi_params(parms, shift_direction, device, val_range=None):
    """The DEVICE parameter table of `isr_multi`: int32 [C,12], one row per channel.  parms: 1..3 (threshold, clip_range,
    shift_pixel) tuples under the one `val_range`, or the reference's dicts (then `val_range` is taken from them).  Threshold and
    clip range are scaled by the log span exactly as `isr_from_gray` scales them.  Build it once, outside any capture."""
    vr, rows = _isr_multi_rows(parms)
    val_range = vr if val_range is None else val_range
    assert val_range is not None, 'isr_multi_params: val_range is needed with tuple rows'
    assert 1 <= len(rows) <= 3, f'isr_multi: 1..3 channels, got {len(rows)}'
    span = np.log(val_range[1]) - np.log(val_range[0])
    prm = torch.zeros(len(rows), ISR_MULTI_ROW, dtype=torch.int32)
    for c, (thr, clip, shift) in enumerate(rows):
        dirs = isr_dirs(shift_direction, shift)
        prm[c, 0:2] = _f32_bits([float(np.float32(span * thr)), float(np.float32(span * clip))])
        prm[c, 2] = len(dirs)
        prm[c, 3:3 + 2 * len(dirs)] = torch.tensor(dirs, dtype=torch.int32).flatten()
    return prm.to(device)


def isr_multi(gray, val_range, prm_dev, C, window=None, out_size=None, ndir_host=None, window_host=None):
    """C ISR channels of the uint8 gray maps [B,H,W] in one call (three launches): channel c = `isr_from_gray` with row c of
    `prm_dev` (`isr_multi_params`), bit for bit -> fp32 [B,C,OH,OW].  window: optional DEVICE int32 [B,3] rows (x0, y0, flip) with
    out_size = (OH, OW): only that crop of the full result (mirrored when flip) is written; the min / max normalisation stays over the
    whole map.  ndir_host (C ints) / window_host (B rows): the table values as the host knows them, checked before anything is
    launched (the device copies cannot be read without a sync; the kernels clamp them)."""
    check_dev(gray, prm_dev, window)
    B, H, W = gray.shape
    assert gray.dtype == torch.uint8 and prm_dev.dtype == torch.int32 and prm_dev.numel() >= C * ISR_MULTI_ROW
    OH, OW = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if window is not None:
        assert window.dtype == torch.int32 and window.shape == (B, 3)
    mm = torch.empty(B * max(C, 0) * 16, dtype=torch.int32, device=gray.device)
    out = torch.empty(B, max(C, 0), OH, OW, dtype=torch.float32, device=gray.device)
    nd = (ctypes.c_int * len(ndir_host))(*[int(v) for v in ndir_host]) if ndir_host is not None else None
    wh = None
    if window_host is not None:
        flat = [int(v) for row in window_host for v in row]
        wh = (ctypes.c_int * len(flat))(*flat)
    call('cmdax4_isr_multi', ptr(gray), ptr(isr_lut(val_range, gray.device)), ptr(prm_dev), ptr(window), ptr(mm), ptr(out), nd, wh,
         c_i32(B), c_i32(C), c_i32(H), c_i32(W), c_i32(OH), c_i32(OW), stream_of(gray))
    return out


def draw_cow_mask(prop_range=(0.7, 0.7), log_sigma_range=(float(np.log(16)), float(np.log(17))), max_sigma=16):
    """The host decisions of ONE cow_masks call of the loader (datasets/utils.py:174-176 with cityscapes_ic.py:264-265's ranges),
    from torch's CPU generator exactly as the reference consumes it: torch.randn([1]).uniform_(...) twice.  The noise field is NOT
    drawn here (the reference takes it from np.random.normal): the kernel generates its own.  -> dict(p, sigma, max_sigma)."""
    p = torch.randn([1, ]).uniform_(prop_range[0], prop_range[1])
    sigma = torch.exp(torch.randn([1, ]).uniform_(log_sigma_range[0], log_sigma_range[1]))
    return dict(p=p.item(), sigma=sigma.item(), max_sigma=max_sigma)


def cow_mask_params(draws, half_width=None):
    """list of draw_cow_mask dicts -> CPU (taps fp32 [B,K], tf fp32 [B]): gaussian_kernels' unnormalised Gaussians
    (utils.py:155-168) and the threshold factors erfinv(2p - 1) * sqrt 2 (:175), both in torch fp32 as the reference computes them.
    K = 2 * half_width + 1; half_width defaults to the reference's round(max_sigma * 3) * 2 + 1 (97 for max_sigma 16: K = 195)."""
    max_sigma = draws[0]['max_sigma']
    assert all(d['max_sigma'] == max_sigma for d in draws)
    p = torch.tensor([d['p'] for d in draws], dtype=torch.float32)
    sigmas = torch.tensor([d['sigma'] for d in draws], dtype=torch.float32)[:, None]
    tf = torch.erfinv(2 * p - 1) * _ROOT_2
    size = round(max_sigma * 3) * 2 + 1 if half_width is None else int(half_width)
    x = torch.arange(-size, size + 1)[None, :].float()
    y = torch.exp(-0.5 * x ** 2 / sigmas ** 2)
    return (y / (sigmas * _ROOT_2_PI)).contiguous(), tf


def _seed64(seed):
    return ctypes.c_uint64(int(seed) & (2 ** 64 - 1))


def cow_field(B, H, W, seed, offset=0, device=None, offset_dev=None):
    """fp32 [B,H,W]: the noise field `cow_mask` generates for (seed, offset [+ the DEVICE int64 offset_dev]) -- field 3 of the
    stream whose fields 0..2 are `randn_fields`"""
    check_dev(offset_dev)
    dev = offset_dev.device if offset_dev is not None else torch.device(device if device is not None else ('cpu' if L.emulated() else 'cuda'))
    out = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    off, offd = _offset_args(offset, offset_dev)
    call('cmdax4_cow_field', ptr(out), c_i32(B), c_i32(H), c_i32(W), _seed64(seed), off, offd, stream_of(out))
    return out


def cow_mask(isr, taps, tf, field=None, seed=0, offset=0, offset_dev=None, enable=None, out=None, debug=False):
    """isr * cow_masks(...) for the fp32 NCHW [B,C,H,W] ISR (three launches, no host sync): a noise field per sample -- `field`
    fp32 [B,H,W], or generated in the kernel as `cow_field(seed, offset)` -- blurred with the sample's K taps behind reflect padding
    and thresholded at tf * std + mean of the blurred field; the same mask on all C channels.  taps fp32 [B,K] / tf fp32 [B]: DEVICE
    tensors (`cow_mask_params`); enable: optional DEVICE int32 [B] (0 = the sample passes through bit for bit).  Out of place unless
    `out` is given (`out=isr` is allowed).  debug: also return the blurred field fp32 [B,H,W]."""
    check_dev(isr, taps, tf, field, offset_dev, enable, out)
    B, C, H, W = isr.shape
    assert isr.dtype == torch.float32 and taps.dtype == torch.float32 and tf.dtype == torch.float32
    assert taps.dim() == 2 and taps.shape[0] == B and tf.shape == (B,)
    assert enable is None or (enable.dtype == torch.int32 and enable.numel() == B)
    K = taps.shape[1]
    if field is not None:
        assert field.shape == (B, H, W) and field.dtype == torch.float32
    if out is None:
        out = torch.empty_like(isr)
    assert out.shape == isr.shape and out.dtype == torch.float32
    smooth = torch.empty(B, H, W, dtype=torch.float32, device=isr.device) if debug else None
    ws = torch.empty(max(1, L.lib().cmdax4_cow_mask_ws_bytes(B, H, W, K)) // 8 + 1, dtype=torch.float64, device=isr.device)
    off, offd = _offset_args(offset, offset_dev)
    call('cmdax4_cow_mask', ptr(isr), ptr(out), ptr(taps), ptr(tf), ptr(field), ptr(enable), ptr(smooth), ptr(ws), c_i32(B), c_i32(C),
         c_i32(H), c_i32(W), c_i32(K), _seed64(seed), off, offd, stream_of(isr))
    return (out, smooth) if debug else out


# ---- ordered event voxel grid and batched events_norm (voxel_ordered.hip, include/cmda_hip_ext5.h) ------------------------------------
def sample_offsets(offsets):
    """sample offsets (B + 1 ints, host) -> (ctypes int64 array, B)"""
    offs = [int(v) for v in offsets]
    return (ctypes.c_int64 * len(offs))(*offs), len(offs) - 1


def events_voxel_ordered_batch(t, x, y, pol, offsets, bins, H, W):
    """events_to_voxel_grid for B samples, order-preserving: prepared fp32 events concatenated over the batch, `offsets` the B + 1
    host sample boundaries -> fp32 [B,bins,H,W].  Every cell is the sequential fp32 sum of the reference (corner pass, then event
    index): bit-identical to its CPU result and from run to run.  No float atomics; the launch count does not depend on B."""
    check_dev(t, x, y, pol)
    assert t.dtype == x.dtype == y.dtype == pol.dtype == torch.float32
    offs, B = sample_offsets(offsets)
    n_total = t.numel()
    assert B < 1 or offs[B] <= n_total == x.numel() == y.numel() == pol.numel(), 'offsets run past the event arrays'
    grid = torch.empty(max(B, 0), max(bins, 0), max(H, 0), max(W, 0), dtype=torch.float32, device=t.device)
    ws = torch.empty(max(1, L.lib().cmdax5_voxel_ordered_ws_bytes(B, offs[B] if B >= 1 else 0, bins, H, W)) // 8 + 1,
                     dtype=torch.float64, device=t.device)
    call('cmdax5_voxel_ordered', ptr(t), ptr(x), ptr(y), ptr(pol), offs, ptr(grid), ptr(ws), c_i32(B), c_i32(bins), c_i32(H),
         c_i32(W), stream_of(t))
    return grid


def events_to_voxel_grid_ordered(t, x, y, pol, bins, H, W):
    """`events_to_voxel_grid` with the reference's summation order (one sample): fp32 [bins,H,W], bit-identical to the oracle"""
    return events_voxel_ordered_batch(t, x, y, pol, [0, t.numel()], bins, H, W)[0]


def events_norm_batch(grids, clip_ranges, final_range=1.0):
    """`events_norm` on each of the B grids fp32 [B,...] with its own clip range (B host floats), three launches; the statistics
    are reduced in a fixed shape (no float atomics): the result is bit-identical from run to run."""
    check_dev(grids)
    assert grids.dtype == torch.float32
    B = grids.shape[0]
    n = grids[0].numel() if B else 0
    assert len(clip_ranges) == B
    out = torch.empty_like(grids)
    ws = torch.empty(max(1, L.lib().cmdax5_events_norm_ws_bytes(B, n)) // 8 + 1, dtype=torch.float64, device=grids.device)
    clips = (ctypes.c_float * max(B, 1))(*[float(c) for c in clip_ranges])
    call('cmdax5_events_norm_batch', ptr(grids), ptr(out), ptr(ws), c_i32(B), c_i64(n), clips, c_f32(final_range),
         stream_of(grids))
    return out


# ---------------------------------------------------------------------------------------------- sixth ABI table (cmda_hip_ext6.h)
def split_mix_targets(logits_image, logits_events, src_label, classes, thr, top=0, bottom=0):
    """The split train type's targets ('cs2dz_image+raw-isr_split', dacs.py:628-651, :759-763) for both streams in two launches and
    one memset: logits_image / logits_events fp32 NHWC [B,h,w,nc] (the teacher's two outputs), src_label int64 [B,H,W], classes
    int64 [B,K] padded with -1.  Returns (pseudo int64 [2,B,H,W], count int32 [2], mixed int64 [2,B,H,W], weight fp32 [2,B,H,W]);
    index 0 = image, 1 = events.  Each half equals pseudo_label -> pseudo_weight -> class_mix_label / class_mix (against ones) on
    that map, bit for bit."""
    check_dev(logits_image, logits_events, src_label, classes)
    if logits_image.shape != logits_events.shape or logits_image.dtype != torch.float32 or logits_events.dtype != torch.float32:
        raise L.CmdaError('split_mix_targets: two fp32 logit maps of one shape')
    if src_label.dtype != torch.int64 or classes.dtype != torch.int64:
        raise L.CmdaError('split_mix_targets: int64 labels and classes')
    B, h, w, nc = logits_image.shape
    _, H, W = src_label.shape
    if src_label.shape[0] != B or classes.dim() != 2 or classes.shape[0] != B:
        raise L.CmdaError('split_mix_targets: labels [B,H,W] and classes [B,K] of the logits\' batch')
    dev = logits_image.device
    pseudo = torch.empty(2, B, H, W, dtype=torch.int64, device=dev)
    mixed = torch.empty(2, B, H, W, dtype=torch.int64, device=dev)
    weight = torch.empty(2, B, H, W, dtype=torch.float32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    K = classes.shape[1]
    call('cmdax6_split_targets', ptr(logits_image), ptr(logits_events), ptr(src_label), ptr(classes), ptr(pseudo), ptr(mixed), ptr(count),
         c_i32(B), c_i32(h), c_i32(w), c_i32(H), c_i32(W), c_i32(nc), c_i32(K), c_f32(thr), stream_of(logits_image))
    call('cmdax6_split_weights', ptr(count), ptr(src_label), ptr(classes), ptr(weight), c_i32(B), c_i32(H), c_i32(W), c_i32(K),
         c_i32(top), c_i32(bottom), stream_of(logits_image))
    return pseudo, count, mixed, weight


# ---------------------------------------------------------------------------------------------- seventh ABI table (cmda_hip_ext7.h)
OHEM_THRESH, OHEM_LOSS = 0, 1


def _ohem_ws(n_keys, device):
    nbytes = L.lib().cmdax7_ws_bytes(n_keys)
    if nbytes < 0:
        raise L.CmdaError(f'cmdax7_ws_bytes: {n_keys} keys are beyond 2^31 - 1')
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def select_kth(keys, k):
    """The k-th smallest (from 0) of an fp32 tensor of any shape, exactly: a 1-element fp32 tensor equal to
    keys.flatten().sort()[0][k].  k: int32 device scalar tensor, read on the device (clamped to [0, n - 1]); nothing synchronises with
    the host.  Radix select, 4 launches and the clearing of its counters."""
    check_dev(keys, k)
    if keys.dtype != torch.float32 or k.dtype != torch.int32 or k.numel() != 1:
        raise L.CmdaError('select_kth: fp32 keys and a 1-element int32 k')
    if L.emulated() and k.is_cuda or (not L.emulated() and k.device != keys.device):
        raise L.CmdaError('select_kth: k on another device than the keys')
    out = torch.empty(1, dtype=torch.float32, device=keys.device)
    ws = _ohem_ws(0, keys.device)
    call('cmdax7_select_kth', ptr(keys), c_i64(keys.numel()), ptr(k), ptr(out), ptr(ws), stream_of(keys))
    return out


def ohem_weight(logits, label, H, W, thresh, min_kept, ignore_index=255, debug=False):
    """OHEMPixelSampler.sample (mmseg/core/seg/sampler/ohem_pixel_sampler.py:32-78) on the low-resolution logits: fp32 NHWC
    [B,h,w,nc] -> fp32 0/1 weights [B,H,W] of the hard pixels among the valid ones (label int64 [B,H,W]; ignore_index and labels
    outside [0, nc) are invalid).  The scores are the bilinear up-sample ce_upsample_fwd sees, bit for bit.
    thresh a float: hard = probability of the label below max(thresh, the min(min_kept * B, n_valid - 1)-th smallest probability);
    thresh None: hard = loss at or above the (min_kept * B)-th largest per-pixel cross-entropy (every valid pixel when there are no
    more than that; pixels that tie with that loss exactly are all taken).
    Nothing here depends on a device value on the host: safe under graph capture.
    debug=True: returns (weight, keys fp32 [B,H,W] with NaN at invalid pixels, threshold fp32 [1])."""
    check_dev(logits, label)
    if logits.dtype != torch.float32 or logits.dim() != 4:
        raise L.CmdaError('ohem_weight: fp32 NHWC logits [B,h,w,nc]')
    B, h, w, nc = logits.shape
    if label.dtype != torch.int64 or tuple(label.shape) != (B, H, W):
        raise L.CmdaError(f'ohem_weight: int64 labels [{B},{H},{W}], got {label.dtype} {tuple(label.shape)}')
    dev = logits.device
    n = B * H * W
    weight = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    thr_out = torch.empty(1, dtype=torch.float32, device=dev) if debug else None
    ws = _ohem_ws(n, dev)
    mode = OHEM_LOSS if thresh is None else OHEM_THRESH
    call('cmdax7_ohem_weight', ptr(logits), ptr(label), ptr(weight), ptr(thr_out), ptr(ws), c_i32(B), c_i32(h), c_i32(w), c_i32(H),
         c_i32(W), c_i32(nc), c_i32(ignore_index), c_i32(mode), c_f32(0.0 if thresh is None else thresh), c_i32(max(-1, min(int(min_kept), 2 ** 31 - 1))),
         stream_of(logits))
    if not debug:
        return weight
    first = L.lib().cmdax7_ws_bytes(0) // 4
    keys = ws[first:first + n].view(torch.float32).view(B, H, W)
    return weight, keys, thr_out


# ---------------------------------------------------------------------------------------------- eighth ABI table (cmda_hip_ext8.h)
_RES_BRANCHES = ('image', 'events')


def _resavg_levels(levels, groups, backward):
    """levels: per feature level dict(image=branch, events=branch, M=rows per group, C=channels, out= (forward) / dout= (backward)),
    branch = dict(z, x, mean, rstd, gamma, beta) (+ dgamma, dbeta in the backward).  Returns (descriptor array, tensors kept alive,
    the per-level ((dz, dres), (dz, dres)) of the backward)"""
    if not 1 <= len(levels) <= 4:
        raise L.CmdaError(f'resavg: 1 to 4 levels, got {len(levels)}')
    arr = (L.Level8 * len(levels))()
    keep, grads = [], []
    first = levels[0]['image']['z']
    for d, lv in zip(arr, levels):
        M, C = int(lv['M']), int(lv['C'])
        io = lv['dout' if backward else 'out']
        maps = [io]
        pair = []
        for b, name in zip(d.br, _RES_BRANCHES):
            br = lv[name]
            maps += [br['z'], br['x']]
            stats = [br['mean'], br['rstd'], br['gamma'], br['beta']] + ([br['dgamma'], br['dbeta']] if backward else [])
            check_dev(*stats)
            if any(t.dtype != torch.float32 for t in stats) or br['mean'].numel() != groups * C or br['rstd'].numel() != groups * C \
                    or any(t.numel() != C for t in stats[2:]):
                raise L.CmdaError('resavg: mean / rstd fp32 [groups, C], gamma / beta (and their gradients) fp32 [C]')
            b.z, b.x, b.mean, b.rstd, b.gamma, b.beta = (t.data_ptr() for t in (br['z'], br['x'], *stats[:4]))
            if backward:
                dz, dres = torch.empty_like(br['z']), torch.empty_like(br['z'])
                b.dz, b.dres, b.dgamma, b.dbeta = dz.data_ptr(), dres.data_ptr(), br['dgamma'].data_ptr(), br['dbeta'].data_ptr()
                pair.append((dz, dres))
                keep += [dz, dres]
            keep += stats
        check_dev(*maps)
        if any(t.dtype != first.dtype or t.numel() != groups * M * C for t in maps):
            raise L.CmdaError(f'resavg: every map holds groups*M*C = {groups * M * C} elements of one storage type')
        if backward:
            d.dout = io.data_ptr()
        else:
            d.out = io.data_ptr()
        d.M, d.C = M, C
        keep += maps
        grads.append(tuple(pair))
    return arr, keep, grads


def resavg_fwd(levels, groups=1):
    """cmdax8_resavg_fwd: lv['out'] = 0.5 * (relu(bn_i(z_i) + x_i) + relu(bn_e(z_e) + x_e)) for up to four levels in ONE launch;
    rows [g*M, (g+1)*M) of a level use row g of mean / rstd.  `out` may be a row slice of a larger buffer.  Returns the outs."""
    arr, keep, _ = _resavg_levels(levels, groups, False)
    first = levels[0]['image']['z']
    call('cmdax8_resavg_fwd', arr, c_i32(len(levels)), c_i32(groups), dtype_tag(first), stream_of(first))
    return [lv['out'] for lv in levels]


def resavg_bwd(levels, groups=1):
    """cmdax8_resavg_bwd (one reducing and one applying launch for all levels, masks recomputed): per level
    ((dz_image, dres_image), (dz_events, dres_events)); dgamma / dbeta of every branch are added into."""
    arr, keep, grads = _resavg_levels(levels, groups, True)
    first = levels[0]['image']['z']
    n = L.lib().cmdax8_ws_floats(arr, len(levels), groups)
    if n < 0:
        raise L.CmdaError('cmdax8_ws_floats: bad shape')
    ws = torch.empty(n, dtype=torch.float32, device=first.device)
    call('cmdax8_resavg_bwd', arr, c_i32(len(levels)), c_i32(groups), ptr(ws), dtype_tag(first), stream_of(first))
    return grads


def bn_stats(x, running_mean, running_var, M, C, eps, momentum, groups=1, order=None, stats_ws=None):
    """cmdax8_bn_stats: the statistics half of bn_train_fwd (same M = rows PER GROUP, groups, order, stats_ws): mean, rstd
    [groups, C], running statistics (may be None) updated; no map is written"""
    check_dev(x, running_mean, running_var, stats_ws)
    mean = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    ws = stats_ws if stats_ws is not None else torch.empty(groups * L.lib().cmda_bn_ws_floats(C), dtype=torch.float32, device=x.device)
    order_c = (ctypes.c_int * groups)(*order) if order is not None else None
    call('cmdax8_bn_stats', ptr(x), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var), ptr(ws), c_i64(M), c_i32(C), c_f32(eps),
         c_f32(momentum), c_i32(groups), order_c, c_i32(int(stats_ws is not None)), dtype_tag(x), stream_of(x))
    return mean, rstd
