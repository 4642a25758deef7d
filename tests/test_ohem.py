"""The OHEM pixel sampler on the device (include/cmda_hip_ext7.h, cmda_amd/csrc/ohem.hip, ops.select_kth / ops.ohem_weight,
decode_heads.OHEMPixelSampler, `sampler=` of the decode heads).

  * ops.select_kth is EXACT: torch.equal against torch.sort.
  * ops.ohem_weight against the reference's own OHEMPixelSampler.sample (tests/golden/ohem.npz, written by
    tests/golden/make_golden_ohem.py) and against a float64 restatement written out below (F.interpolate bilinear,
    align_corners=False, softmax / cross-entropy, gather, sort -- what the reference does, in float64).

Comparison rule.  The kernel computes its keys in fp32 with the fast exp / log of ce_fwd_kernel, so a pixel whose key lies within
rounding of the threshold may fall on either side.  Keys and the threshold must lie within KEY_TOL of float64; the weight map must
equal the checker's EXACTLY outside the band |key - threshold| <= 2 KEY_TOL; the band may hold at most 0.1 % of the valid pixels
(one pixel for maps below 1000 pixels).  The band share is a property of the inputs: it is asserted on the float64 restatement alone
before the kernel's output is looked at.

KEY_TOL = 8 x the distance of the REFERENCE's own fp32 computation (torch's fp32 F.interpolate, softmax / log_softmax and gather on
the CPU) from the float64 restatement, per input and per kind of key: the table REF_DIST below, printed by `python tests/test_ohem.py`
(`_reference_fp32_distance`).  Probability keys 1.3e-7 ... 2.9e-7, loss keys 0.6e-6 ... 1.7e-6 on the inputs whose up-sampling ratio
is 1 or 4; ten times that (2.8e-6 / 2.1e-5) on the 10 x 18 -> 37 x 70 map, where a ratio that is no power of two puts the rounding of the
fp32 source coordinate into every bilinear weight.  ("Row statistics over their range", bounds ce_fwd_kernel's lse
for the ratios 1, 2 and 4 only, so the constants are not derived from that row.)  test_key_tol_follows_the_reference_distance
recomputes the distances and holds the table to them.
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
if os.path.dirname(HERE) not in sys.path:   # (run as a script, to print REF_DIST)
    sys.path.insert(0, os.path.dirname(HERE))
from weights import DACS_SEG_SCALE, seeded_fill  # noqa: E402

import cmda_amd.runtime as rt  # noqa: E402
import test_dacs as TD  # noqa: E402
import test_split_uda as TS  # noqa: E402
from cmda_amd import _lib as L  # noqa: E402
from cmda_amd import ops  # noqa: E402
from cmda_amd.registry import build_train_model  # noqa: E402
from conftest import assert_close, check_ge, check_le  # noqa: E402

# input -> (probability keys, loss keys): max |reference fp32 - float64| over the valid pixels
REF_DIST = {'x4': (2.940e-7, 1.282e-6), 'ragged': (2.814e-6, 2.138e-5), 'one_tile_row': (2.709e-7, 1.734e-6), 'nc2': (1.347e-7, 5.539e-7),
            'nc32': (2.749e-7, 1.286e-6), 'golden': (1.716e-7, 1.055e-6)}


def key_tol(name, thresh):
    return 8 * REF_DIST[name][1 if thresh is None else 0]


# ---------------------------------------------------------------------------------------------------------------------------
# select_kth: exact
SEL_N = [1, 2, 63, 64, 65, 2047, 2049, 40003]


def _key_family(name, n):
    g = torch.Generator().manual_seed(300 + n)
    if name == 'all_equal':
        return torch.full((n,), 0.3125)
    if name == 'two_values':
        return torch.where(torch.rand(n, generator=g) < 0.4, torch.tensor(0.25), torch.tensor(0.75))
    if name == 'lowest_bit':   # 1.0 and its successor: one bucket until the last level, where they part
        bits = torch.full((n,), 0x3F800000, dtype=torch.int32) + (torch.rand(n, generator=g) < 0.5).int()
        return bits.view(torch.float32)
    if name == 'exponents':    # denormals to 1e30
        e = torch.rand(n, generator=g, dtype=torch.float64) * 75.0 - 45.0
        x = (10.0 ** e).float()
        x[::7] = torch.tensor(1e-45)   # the smallest denormal
        return x
    if name == 'zero_and_tiny':
        x = torch.rand(n, generator=g) * 1e-38
        x[torch.rand(n, generator=g) < 0.5] = 0.0
        return x
    if name == 'negatives':
        return torch.randn(n, generator=g) * torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(1e-6), torch.tensor(5.0))
    if name == 'inf_tail':
        x = torch.rand(n, generator=g)
        x[n - (n + 3) // 4:] = float('inf')
        return x
    raise KeyError(name)


FAMILIES = ['all_equal', 'two_values', 'lowest_bit', 'exponents', 'zero_and_tiny', 'negatives', 'inf_tail']


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('n', SEL_N)
def test_select_kth_is_exact(tgt, n, family):
    x = _key_family(family, n)
    srt = x.sort()[0]
    keys = tgt.to(x)
    for k in sorted({0, min(1, n - 1), n // 2, max(n - 2, 0), n - 1}):
        kd = tgt.to(torch.tensor(k, dtype=torch.int32))
        got = ops.select_kth(keys, kd)
        assert got.shape == (1,) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), srt[k:k + 1]), f'n {n}, k {k}: {got.item()!r} against {srt[k].item()!r}'
        again = ops.select_kth(keys, kd)
        assert torch.equal(again.cpu().view(torch.int32), got.cpu().view(torch.int32)), 'run-to-run bit equality'
    assert torch.equal(keys.cpu(), x), 'the keys are not modified'


def test_select_kth_any_shape_and_clamped_k(tgt):
    x = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(5))
    srt = x.flatten().sort()[0]
    for k, want in ((52, 52), (-3, 0), (105, 104), (1 << 30, 104)):
        got = ops.select_kth(tgt.to(x), tgt.to(torch.tensor([k], dtype=torch.int32)))
        assert torch.equal(got.cpu(), srt[want:want + 1]), k


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 restatement of OHEMPixelSampler.sample on low-resolution logits
def restate(logits_nhwc, label, thresh, min_kept, ignore_index=255, dtype=torch.float64):
    """-> (key [B,H,W], threshold (float), weight bool [B,H,W], valid bool [B,H,W]); dtype float32 = the reference's own arithmetic"""
    B, H, W = label.shape
    nc = logits_nhwc.shape[-1]
    up = F.interpolate(logits_nhwc.permute(0, 3, 1, 2).to(dtype), size=(H, W), mode='bilinear', align_corners=False)
    valid = (label != ignore_index) & (label >= 0) & (label < nc)
    safe = torch.where(valid, label, torch.zeros_like(label)).unsqueeze(1)
    batch_kept = min_kept * B
    n_valid = int(valid.sum())
    if thresh is not None:
        key = F.softmax(up, dim=1).gather(1, safe).squeeze(1)
        srt = key[valid].sort()[0]
        thr = max(srt[min(batch_kept, n_valid - 1)].item(), thresh) if n_valid else thresh
        weight = valid & (key < thr)
    else:
        key = -F.log_softmax(up, dim=1).gather(1, safe).squeeze(1)
        srt = key[valid].sort(descending=True)[0]
        thr = srt[min(batch_kept, n_valid) - 1].item() if n_valid else float('inf')
        weight = valid & (key >= thr)
    return key, thr, weight, valid


def compare(name, run, checker, tol):
    """the comparison rule of the file header.  run: () -> (weight, keys, threshold) of the kernel; checker: (key64, thr64, weight, valid)
    with `weight` the map to equal outside the band (the restatement's or the reference's)"""
    key64, thr64, want, valid = checker
    n_valid = int(valid.sum())
    band = valid & ((key64 - thr64).abs() <= 2 * tol) if np.isfinite(thr64) else torch.zeros_like(valid)
    allowed = max(1e-3 * n_valid, 1.0 if n_valid < 1000 else 0.0)
    check_le(f'{name}: pixels within 2 KEY_TOL of the threshold (a condition on the inputs)', int(band.sum()), allowed)
    weight, keys, thr = [t.cpu() for t in run()]
    if n_valid:
        check_le(f'{name}: key error', (keys[valid].double() - key64[valid].double()).abs().max().item(), tol)
    if np.isfinite(thr64):
        check_le(f'{name}: threshold error', abs(thr.item() - thr64), tol)
    else:
        assert thr.item() == thr64
    assert bool(((weight == 0) | (weight == 1)).all()) and not bool(weight[~valid].any()), f'{name}: 0 / 1 weights, 0 at invalid pixels'
    assert bool(keys[~valid].isnan().all()), f'{name}: invalid pixels carry no key'
    assert torch.equal(weight[~band], want[~band].float()), f'{name}: {int((weight[~band] != want[~band].float()).sum())} pixels outside the band differ'
    return weight, keys, thr


# (thresh, min_kept as a share of the pixels of ONE sample or an absolute count)
SETTINGS = {'thresh_wins': (0.7, 2), 'kth_wins': (0.02, 0.6), 'kth_last': (0.7, 100000), 'loss_tenth': (None, 0.1), 'loss_all': (None, 100000)}
# (B, h, w, H, W, nc)
SHAPES = {'x4': (2, 16, 24, 64, 96, 19), 'ragged': (2, 10, 18, 37, 70, 19), 'one_tile_row': (2, 3, 3, 8, 130, 19),
          'nc2': (2, 8, 8, 32, 32, 2), 'nc32': (2, 8, 8, 32, 32, 32)}
# seeds for which every setting has at most 0.1 % of its valid pixels within 2 KEY_TOL of the float64 threshold (asserted in `compare`)
INPUT_SEED = {'x4': 535, 'ragged': 507, 'one_tile_row': 443, 'nc2': 479, 'nc32': 496}
_CACHE = {}


def _min_kept(mk, H, W):
    return mk if isinstance(mk, int) else max(2, int(mk * H * W))


def up_inputs(shape):
    """seeded low-resolution logits (scale 3, spread so that the label's probability covers (0, 1)) and labels with ~5 % of 255"""
    if shape not in _CACHE:
        B, h, w, H, W, nc = SHAPES[shape]
        g = torch.Generator().manual_seed(INPUT_SEED[shape])
        lg = torch.randn(B, h, w, nc, generator=g) * 3
        lab = F.interpolate(lg.permute(0, 3, 1, 2), size=(H, W), mode='nearest').argmax(1)   # the likely class ...
        rnd = torch.randint(0, nc, (B, H, W), generator=g)
        lab = torch.where(torch.rand(B, H, W, generator=g) < 0.5, lab, rnd)                   # ... or any class, half and half
        lab[torch.rand(B, H, W, generator=g) < 0.05] = 255
        _CACHE[shape] = (lg, lab.contiguous(), {})
    return _CACHE[shape]


def up_checker(shape, setting):
    lg, lab, memo = up_inputs(shape)
    if setting not in memo:
        thresh, mk = SETTINGS[setting]
        memo[setting] = restate(lg, lab, thresh, _min_kept(mk, *SHAPES[shape][3:5]))
    return memo[setting]


@pytest.mark.parametrize('setting', list(SETTINGS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_ohem_weight_matches_float64_restatement(tgt, shape, setting):
    B, h, w, H, W, nc = SHAPES[shape]
    lg, lab, _ = up_inputs(shape)
    thresh, mk = SETTINGS[setting]
    mk = _min_kept(mk, H, W)
    key64, thr64, want, valid = up_checker(shape, setting)
    n_valid, kept = int(valid.sum()), int(want.sum())
    # the setting is in the regime it is named for
    if setting == 'thresh_wins':
        assert thr64 == thresh and 0 < kept < n_valid
    elif setting == 'kth_wins':
        assert thr64 > thresh and kept == mk * B
    elif setting == 'kth_last':
        assert thr64 > thresh and n_valid - 3 <= kept < n_valid
    elif setting == 'loss_tenth':
        assert kept == mk * B < n_valid
    else:
        assert kept == n_valid
    tol = key_tol(shape, thresh)
    weight, _, _ = compare(f'{shape} {setting}', lambda: ops.ohem_weight(tgt.to(lg), tgt.to(lab), H, W, thresh, mk, debug=True),
                           (key64, thr64, want, valid), tol)
    plain = ops.ohem_weight(tgt.to(lg), tgt.to(lab), H, W, thresh, mk)
    assert torch.equal(plain.cpu(), weight), 'debug=False returns the same map'


def _reference_fp32_distance():
    """the reference's own fp32 arithmetic against the float64 restatement on every input of this file (no kernel involved)"""
    cases = {s: up_inputs(s)[:2] for s in SHAPES}
    g = golden()
    cases['golden'] = (g['logits'].permute(0, 2, 3, 1).contiguous(), g['label'][:, 0].long())
    out = {}
    for name, (lg, lab) in cases.items():
        d = []
        for thresh in (0.5, None):
            k64, _, _, valid = restate(lg, lab, thresh, 2)
            k32 = restate(lg, lab, thresh, 2, dtype=torch.float32)[0]
            d.append((k32.double() - k64)[valid].abs().max().item())
        out[name] = tuple(d)
    return out


def test_key_tol_follows_the_reference_distance():
    """REF_DIST is what it says: within a quarter of the distances recomputed here (torch's fp32 kernels differ a little between CPUs)"""
    dist = _reference_fp32_distance()
    assert set(dist) == set(REF_DIST)
    for name, d in dist.items():
        for i, kind in enumerate(('probability', 'loss')):
            check_le(f'{name}: recorded fp32 reference distance, {kind} keys, over the recomputed one', REF_DIST[name][i] / d[i], 1.25)
            check_ge(f'{name}: recorded fp32 reference distance, {kind} keys, over the recomputed one', REF_DIST[name][i] / d[i], 0.8)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own sampler (tests/golden/ohem.npz)
GOLDEN_SETTINGS = {'thresh_wins': (0.7, 2), 'kth_wins': (0.05, 500), 'kth_last': (0.7, 100000), 'loss_300': (None, 300), 'loss_all': (None, 100000)}


def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, 'golden', 'ohem.npz')).items()}


@pytest.mark.parametrize('setting', list(GOLDEN_SETTINGS))
def test_ohem_weight_matches_reference_sampler(tgt, setting):
    g = golden()
    thresh, mk = GOLDEN_SETTINGS[setting]
    lg = g['logits'].permute(0, 2, 3, 1).contiguous()   # [2,24,32,19]: the labels' resolution (scale 1)
    lab = g['label'][:, 0].long().contiguous()
    B, H, W = lab.shape
    key64, thr64, w64, valid = restate(lg, lab, thresh, mk)
    want = g['weight.' + setting].bool()
    tol = key_tol('golden', thresh)
    band = valid & ((key64 - thr64).abs() <= 2 * tol)
    assert torch.equal(want[~band], w64[~band]), 'the restatement restates the reference'
    compare(f'golden {setting}', lambda: ops.ohem_weight(tgt.to(lg), tgt.to(lab), H, W, thresh, mk, debug=True), (key64, thr64, want, valid), tol)
    # the same through the reference's signature (NCHW logits, label [B,1,H,W]) with a head-like context
    from cmda_amd import decode_heads as dh

    class Ctx:
        ignore_index = 255
    ctx = Ctx()   # (the sampler holds its context weakly)
    sampler = dh.OHEMPixelSampler(ctx, thresh=thresh, min_kept=mk)
    got = sampler.sample(tgt.to(g['logits']), tgt.to(g['label'].long()))
    assert got.shape == (B, H, W)
    assert torch.equal(got.cpu(), ops.ohem_weight(tgt.to(lg), tgt.to(lab), H, W, thresh, mk).cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# edge cases
@pytest.mark.parametrize('thresh', [0.7, None], ids=['thresh', 'loss'])
def test_ohem_every_label_ignored(tgt, thresh):
    lg, lab, _ = up_inputs('x4')
    B, h, w, H, W, nc = SHAPES['x4']
    weight, keys, thr = ops.ohem_weight(tgt.to(lg), tgt.to(torch.full_like(lab, 255)), H, W, thresh, 100, debug=True)
    assert not bool(weight.cpu().any()) and bool(keys.cpu().isnan().all())
    assert thr.item() == (np.float32(0.7) if thresh is not None else float('inf'))


@pytest.mark.parametrize('thresh', [0.999, 1e-4, None], ids=['thresh_high', 'thresh_low', 'loss'])
def test_ohem_one_valid_pixel(tgt, thresh):
    lg, lab, _ = up_inputs('ragged')
    B, h, w, H, W, nc = SHAPES['ragged']
    one = torch.full_like(lab, 255)
    one[1, 20, 33] = 4
    key64, thr64, want, valid = restate(lg, one, thresh, 100)
    assert int(valid.sum()) == 1 and 1e-4 + 1e-5 < restate(lg, one, 0.5, 100)[0][1, 20, 33].item() < 0.999 - 1e-5
    weight, keys, thr = [t.cpu() for t in ops.ohem_weight(tgt.to(lg), tgt.to(one), H, W, thresh, 100, debug=True)]
    tol = key_tol('ragged', thresh)
    check_le('one valid pixel: key error', abs(keys[1, 20, 33].item() - key64[1, 20, 33].item()), tol)
    check_le('one valid pixel: threshold error', abs(thr.item() - thr64), tol)
    # thresh above the pixel's probability: hard; below: the pixel is its own k-th key and p < p is false; loss mode: it is the top loss
    assert int(weight.sum()) == (0 if thresh == 1e-4 else 1) and weight[1, 20, 33].item() == (0.0 if thresh == 1e-4 else 1.0)
    assert torch.equal(weight, want.float())


@pytest.mark.parametrize('setting', ['thresh_wins', 'kth_wins', 'loss_tenth'])
def test_ohem_out_of_range_labels_are_invalid(tgt, setting):
    """labels such as 40 (>= nc) or -1 take no part: the result is the one with 255 in their place, and CE's kernels agree"""
    B, h, w, H, W, nc = SHAPES['x4']
    lg, lab, _ = up_inputs('x4')
    thresh, mk = SETTINGS[setting]
    mk = _min_kept(mk, H, W)
    g = torch.Generator().manual_seed(9)
    bad = torch.rand(B, H, W, generator=g) < 0.1
    odd = torch.where(bad, torch.where(torch.rand(B, H, W, generator=g) < 0.5, torch.tensor(40), torch.tensor(-1)), lab)
    clean = torch.where(bad, torch.tensor(255), lab)
    a = ops.ohem_weight(tgt.to(lg), tgt.to(odd), H, W, thresh, mk, debug=True)
    b = ops.ohem_weight(tgt.to(lg), tgt.to(clean), H, W, thresh, mk, debug=True)
    assert not bool(a[0].cpu()[bad].any()) and bool(a[1].cpu()[bad].isnan().all())
    assert torch.equal(a[0].cpu(), b[0].cpu()) and torch.equal(a[2].cpu(), b[2].cpu())
    compare(f'out-of-range labels, {setting}', lambda: a, restate(lg, odd, thresh, mk), key_tol('x4', thresh))


def test_ohem_loss_mode_takes_every_tie_at_the_boundary(tgt):
    """two pixels fed identical logits and labels tie exactly; where batch_kept falls between them, both are selected (the reference's
    unstable sort would keep one of them, unspecified which)"""
    B, h, w, nc = 1, 8, 6, 19   # scale 1: a pixel's key is a function of its own logits and label
    g = torch.Generator().manual_seed(21)
    lg = torch.randn(B, h, w, nc, generator=g)
    lab = torch.randint(0, nc, (B, h, w), generator=g)
    order = restate(lg, lab, None, 2)[0].flatten().argsort(descending=True)
    first, second = order[4].item(), order[5].item()   # four losses above them; the pair becomes ranks 4 and 5
    lgf, labf = lg.view(-1, nc).clone(), lab.flatten().clone()
    lgf[second], labf[second] = lgf[first], labf[first]
    lg, lab = lgf.view(B, h, w, nc).contiguous(), labf.view(B, h, w).contiguous()
    key = restate(lg, lab, None, 2)[0].flatten()
    assert key[first] == key[second] and int((key > key[first]).sum()) == 4 and int((key == key[first]).sum()) == 2
    for min_kept, taken in ((4, 4), (5, 6), (6, 6), (7, 7)):
        weight, keys, thr = [t.cpu().flatten() for t in ops.ohem_weight(tgt.to(lg), tgt.to(lab), h, w, None, min_kept, debug=True)]
        assert keys[first].item() == keys[second].item(), 'identical inputs, identical keys'
        assert int(weight.sum()) == taken, f'min_kept {min_kept}: {int(weight.sum())} pixels'
        assert weight[first].item() == weight[second].item() == (0.0 if min_kept == 4 else 1.0)
        if min_kept in (5, 6):
            assert thr.item() == keys[first].item(), 'the boundary is the tied key'


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
def _raw(name, *args):
    return getattr(L.lib(), name)(*args)


def test_seventh_table_refusals(tgt):
    """every refusal is decided on the host before the launch: nothing is written"""
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    SHAPE, UNSUPPORTED = -1, -4
    B, h, w, H, W, nc = 1, 2, 2, 8, 8, 3
    lg = tgt.to(torch.randn(B, h, w, nc))
    lab = tgt.to(torch.zeros(B, H, W, dtype=torch.int64))
    weight = tgt.to(torch.full((B, H, W), 7.0))
    thr = tgt.to(torch.full((1,), 7.0))
    nws = L.lib().cmdax7_ws_bytes(B * H * W) // 4
    assert L.lib().cmdax7_ws_bytes(0) > 0 and nws * 4 == L.lib().cmdax7_ws_bytes(0) + 4 * B * H * W
    assert L.lib().cmdax7_ws_bytes(-1) == -1 and L.lib().cmdax7_ws_bytes(1 << 31) == -1
    ws = tgt.to(torch.full((nws,), 7, dtype=torch.int32))
    keys = tgt.to(torch.full((16,), 7.0))
    kd = tgt.to(torch.zeros(1, dtype=torch.int32))
    out = tgt.to(torch.full((1,), 7.0))
    p = L.ptr

    def ohem(l=lg, lb=lab, wt=weight, t=thr, s=ws, B=B, h=h, w=w, H=H, W=W, nc=nc, mode=0, min_kept=2):
        return _raw('cmdax7_ohem_weight', p(l), p(lb), p(wt), p(t), p(s), i32(B), i32(h), i32(w), i32(H), i32(W), i32(nc), i32(255),
                    i32(mode), f32(0.7), i32(min_kept), None)

    def select(ks=keys, n=16, k=kd, o=out, s=ws):
        return _raw('cmdax7_select_kth', p(ks), i64(n), p(k), p(o), p(s), None)

    for kw in (dict(nc=0), dict(nc=33), dict(nc=-1), dict(B=0), dict(h=0), dict(w=0), dict(H=0), dict(W=-1), dict(min_kept=1),
               dict(min_kept=0), dict(min_kept=-5), dict(B=2, H=1 << 15, W=1 << 15), dict(B=1 << 11, H=1 << 10, W=1 << 10)):
        assert ohem(**kw) == SHAPE, kw
    for kw in (dict(l=None), dict(lb=None), dict(wt=None), dict(s=None), dict(mode=2), dict(mode=-1)):
        assert ohem(**kw) == UNSUPPORTED, kw
    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 31)):
        assert select(**kw) == SHAPE, kw
    for kw in (dict(ks=None), dict(k=None), dict(o=None), dict(s=None)):
        assert select(**kw) == UNSUPPORTED, kw
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    for t in (weight, thr, out, keys):
        assert bool((t.cpu() == 7.0).all()), 'a refused call wrote'
    assert bool((ws.cpu() == 7).all()), 'a refused call wrote into the workspace'
    # legal: 32 classes are the most, min_kept = 2 the least, the threshold output may be left out
    lg32 = tgt.to(torch.randn(B, h, w, 32))
    assert ohem(l=lg32, nc=32, t=None) == 0 and ohem(mode=1) == 0 and select() == 0
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()
    assert out.item() == 7.0 and bool(((weight.cpu() == 0) | (weight.cpu() == 1)).all())
    # the Python ops refuse what the table cannot describe, and pass the table's refusals on
    with pytest.raises(L.CmdaError):
        ops.ohem_weight(lg, lab, H, W, 0.7, 1)
    with pytest.raises(L.CmdaError):
        ops.ohem_weight(lg, lab.int(), H, W, 0.7, 2)
    with pytest.raises(L.CmdaError):
        ops.ohem_weight(lg, lab, H + 1, W, 0.7, 2)
    with pytest.raises(L.CmdaError):
        ops.ohem_weight(lg.double(), lab, H, W, 0.7, 2)
    with pytest.raises(L.CmdaError):
        ops.select_kth(keys, kd.long())
    with pytest.raises(L.CmdaError):
        ops.select_kth(keys[:0], kd)


# ---------------------------------------------------------------------------------------------------------------------------
# decode heads.  Labels cover ONE 64 x 8 tile of one sample, so that each cross-entropy sum is one workgroup's (the loss kernel adds one
# partial per workgroup with a float atomic: over several the order is free) and losses can be compared bit for bit.
SAMPLER = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=64)
HB, HH, HW = 1, 8, 64


def _head_gt(seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, 19, (HB, 1, HH, HW), generator=g)
    gt[torch.rand(HB, 1, HH, HW, generator=g) < 0.1] = 255
    return gt, torch.rand(HB, HH, HW, generator=g)


def _plain_head(tgt, **kw):
    from cmda_amd import decode_heads as dh
    rt.set_compute_dtype(torch.float32)
    head = dh.DAFormerHead(**dict(TS.HEAD_KW, **kw), decoder_params=TS.decoder_params())
    seeded_fill(head, 51)
    with torch.no_grad():
        head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    return head.train().to(tgt.device)


def _fusion_head(tgt, **kw):
    from cmda_amd import decode_heads as dh
    rt.set_compute_dtype(torch.float32)
    head = dh.DAFormerHeadFusion(**dict(TS.HEAD_KW, **kw), decoder_params=TS.decoder_params(train_type='cs2dsec_image+events_together', share_decoder=True))
    seeded_fill(head, 51)
    with torch.no_grad():
        head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    return head.train().to(tgt.device)


def _sampler_weight(logits, gt):
    w = ops.ohem_weight(logits, gt.view(HB, HH, HW), HH, HW, SAMPLER['thresh'], SAMPLER['min_kept'])
    assert 0 < int(w.sum().item()) < HB * HH * HW
    return w


@pytest.mark.parametrize('mode', ['thresh', 'loss'])
def test_head_with_sampler_equals_ce_with_the_ohem_weight(tgt, mode):
    from cmda_amd import decode_heads as dh
    sampler = dict(SAMPLER) if mode == 'thresh' else dict(type='OHEMPixelSampler', min_kept=100)
    head = _plain_head(tgt, sampler=sampler)
    assert isinstance(head.sampler, dh.OHEMPixelSampler) and head.sampler.context is head and 'sampler' not in dict(head.named_modules())
    feats = TS.feats_nlc(tgt, HB, 32, 256, 52, 'i')
    gt, wt = _head_gt(53)
    gt, wt = tgt.to(gt), tgt.to(wt)
    losses, logits, saved = head.fwd_train(feats, HB, gt, wt)   # the incoming weight is ignored
    w = ops.ohem_weight(logits, gt.view(HB, HH, HW), HH, HW, sampler.get('thresh'), sampler['min_kept'])
    assert 0 < int(w.sum().item()) < HB * HH * HW
    loss, acc, sv = dh.ce_losses_fwd(logits, gt, w, head.ignore_index, 1.0)
    assert torch.equal(losses['loss_seg'].cpu(), loss.cpu()) and torch.equal(losses['acc_seg'].cpu(), acc.cpu())
    assert torch.equal(saved[1][2].cpu(), w.cpu()), 'the weight saved for the backward is the sampler\'s'
    other, _, _ = head.fwd_train(feats, HB, gt, None)
    assert torch.equal(other['loss_seg'].cpu(), loss.cpu()), 'with or without an incoming weight'
    caught = {}
    head.bwd = lambda sv_, dl, B_: caught.setdefault('dl', dl)
    head.bwd_train(saved, HB, mul=0.5)
    ref = dh.ce_losses_bwd(sv, None, 0.5, head.ignore_index, 1.0)
    assert torch.equal(caught['dl'].cpu(), ref.cpu()) and bool(ref.abs().sum().item() > 0)
    # and the plain loss is another one
    plain, _, _ = dh.ce_losses_fwd(logits, gt, wt, head.ignore_index, 1.0)
    assert not torch.equal(plain.cpu(), loss.cpu())


def test_head_without_sampler_is_unchanged(tgt):
    feats = TS.feats_nlc(tgt, HB, 32, 256, 52, 'i')
    gt, wt = _head_gt(53)
    gt, wt = tgt.to(gt), tgt.to(wt)
    outs = []
    for kw in (dict(), dict(sampler=None)):
        head = _plain_head(tgt, **kw)
        assert head.sampler is None
        losses, logits, saved = head.fwd_train(feats, HB, gt, wt)
        caught = {}
        head.bwd = lambda sv_, dl, B_, c=caught: c.setdefault('dl', dl)
        head.bwd_train(saved, HB)
        outs.append((losses['loss_seg'].cpu(), losses['acc_seg'].cpu(), logits.cpu(), caught['dl'].cpu(), saved[1][2].cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][4], wt.cpu()), 'the caller\'s weight is the one used'


def _fusion_inputs(tgt):
    return {k: TS.feats_nlc(tgt, HB, 32, 256, 52, k) for k in ('f_image', 'f_events', 'f_fusion', 'f_img_self_res')}


def test_fusion_head_loss_mix_takes_each_terms_own_weight(tgt):
    from cmda_amd import decode_heads as dh
    head = _fusion_head(tgt, sampler=dict(SAMPLER))
    plain = _fusion_head(tgt)
    inputs = _fusion_inputs(tgt)
    gt, wt = _head_gt(53)
    gt, wt = tgt.to(gt), tgt.to(wt)
    cfg = dict(TD.FCFG)
    losses, logits, (saved, sv_l, coef) = head.fwd_train(inputs, HB, gt, wt, cfg)
    _, _, (_, sv_plain, coef_plain) = plain.fwd_train(inputs, HB, gt, wt, cfg)
    assert coef == coef_plain and set(sv_l) == {'image_output', 'events_output', 'fusion_output', 'img_self_res_output'}
    terms, maps = {}, {}
    for k in sv_l:
        assert torch.equal(sv_plain[k][0].cpu(), logits[k].cpu()), 'the sampler leaves the logits alone'
        assert torch.equal(sv_plain[k][2].cpu(), wt.cpu())
        maps[k] = _sampler_weight(logits[k], gt)
        assert torch.equal(sv_l[k][2].cpu(), maps[k].cpu()), f'{k}: the saved weight is the sampler\'s, from this term\'s logits'
        terms[k] = dh.ce_losses_fwd(logits[k], gt, maps[k], head.ignore_index, 1.0)
    assert not torch.equal(maps['image_output'].cpu(), maps['events_output'].cpu()), 'the terms\' hard pixels differ'
    total = None
    for k in ('fusion_output', 'image_output', 'img_self_res_output', 'events_output'):   # the reference's order of additions
        t = terms[k][0] * coef[k]
        total = t if total is None else total + t
    assert torch.equal(losses['loss_seg'].cpu(), total.cpu()) and torch.equal(losses['acc_seg'].cpu(), terms['fusion_output'][1].cpu())
    again, _, _ = head.fwd_train(inputs, HB, gt, None, cfg)
    assert torch.equal(again['loss_seg'].cpu(), total.cpu()), 'an incoming seg_weight is ignored'
    caught = {}
    head.bwd = lambda sv_, dl, B_: caught.update(dl)
    head.bwd_train((saved, sv_l, coef), HB, mul=0.5)
    for k in sv_l:
        ref = dh.ce_losses_bwd(terms[k][2], None, 0.5 * coef[k], head.ignore_index, 1.0)
        assert torch.equal(caught[k].cpu(), ref.cpu()) and bool(ref.abs().sum().item() > 0), k


def test_fusion_head_joint_pass_takes_each_terms_own_weight(tgt):
    from cmda_amd import decode_heads as dh
    head = _fusion_head(tgt, sampler=dict(SAMPLER))
    inputs = _fusion_inputs(tgt)
    names = ('image', 'fusion', 'events', 'isr')
    fkey = {'image': 'f_image', 'fusion': 'f_fusion', 'events': 'f_events', 'isr': 'f_img_self_res'}
    joint = [(torch.cat([inputs[fkey[n]][i][0] for n in names]).contiguous(), inputs['f_image'][i][1], inputs['f_image'][i][2]) for i in range(4)]
    gt, wt = _head_gt(53)
    gt, wt = tgt.to(gt), tgt.to(wt)
    cfg = dict(TD.FCFG)
    losses, logits, (saved, sv_ls, coef) = head.fwd_train_joint(joint, names, HB, gt, wt, cfg)
    n = float(HB * HH * HW)
    L_terms, maps = [], {}
    for nm in names:
        k = head._KEY[nm]
        maps[k] = _sampler_weight(logits[k], gt)
        assert torch.equal(sv_ls[0][k][2].cpu(), maps[k].cpu()), f'{k}: the saved weight is the sampler\'s, from this term\'s logits'
        acc, _ = ops.ce_upsample_fwd(logits[k], gt.view(HB, HH, HW), maps[k], HH, HW, head.ignore_index)
        L_terms.append(acc[0] * (1.0 / n))
    assert not torch.equal(maps['image_output'].cpu(), maps['fusion_output'].cpu())
    cvec = torch.tensor([coef[head._KEY[nm]] for nm in names], dtype=torch.float32).to(tgt.device)
    assert torch.equal(losses['loss_seg'].cpu(), torch.dot(torch.stack(L_terms), cvec).cpu())
    again, _, _ = head.fwd_train_joint(joint, names, HB, gt, None, cfg)
    assert torch.equal(again['loss_seg'].cpu(), losses['loss_seg'].cpu()), 'an incoming seg_weight is ignored'
    caught = {}
    head.bwd_joint = lambda sv_, dl, B_: caught.setdefault('dl', dl)
    head.bwd_train_joint((saved, sv_ls, coef), HB, mul=0.5)
    for g_, nm in enumerate(names):
        k = head._KEY[nm]
        ref = dh.ce_losses_bwd(sv_ls[0][k], None, 0.5 * coef[k], head.ignore_index, 1.0)
        assert torch.equal(caught['dl'][g_ * HB:(g_ + 1) * HB].cpu(), ref.cpu()) and bool(ref.abs().sum().item() > 0), k


def test_split_head_dict_targets_give_each_stream_its_own_weight(tgt):
    head = TS.split_head(tgt, sampler=dict(SAMPLER))
    inputs = {'f_image': TS.feats_nlc(tgt, HB, 32, 256, 52, 'i'), 'f_events': TS.feats_nlc(tgt, HB, 32, 256, 52, 'e')}
    gi, wi = _head_gt(54)
    ge, we = _head_gt(55)
    gts = {'image': tgt.to(gi), 'events': tgt.to(ge)}
    losses, logits, (saved, sv_l, coef) = head.fwd_train(inputs, HB, gts, {'image': tgt.to(wi), 'events': tgt.to(we)}, TS.FCFG)
    for key, stream in (('image_output', 'image'), ('events_output', 'events')):
        want = _sampler_weight(logits[key], gts[stream])
        assert torch.equal(sv_l[key][2].cpu(), want.cpu()), f'{key}: from its own logits and its own stream\'s labels'
        assert not bool(sv_l[key][2].cpu()[gts[stream].cpu().view(HB, HH, HW) == 255].any())
        swapped = _sampler_weight(logits[key], gts['events' if stream == 'image' else 'image'])
        assert not torch.equal(swapped.cpu(), want.cpu())


def test_unknown_sampler_type_raises():
    from cmda_amd import decode_heads as dh
    with pytest.raises(KeyError, match='RandomPixelSampler'):
        dh.DAFormerHead(**dict(TS.HEAD_KW, sampler=dict(type='RandomPixelSampler')), decoder_params=TS.decoder_params())
    with pytest.raises(AssertionError):
        dh.DAFormerHead(**dict(TS.HEAD_KW, sampler=dict(type='OHEMPixelSampler', min_kept=1)), decoder_params=TS.decoder_params())


def test_head_with_sampler_is_freed_with_its_last_reference():
    """no head -> sampler -> head cycle: the head goes when its last name goes (a model waiting for the cyclic collector keeps its
    weight copies alive into a later model's graph capture), and a deep copy's sampler points at the copy"""
    import copy
    import gc
    import weakref
    from cmda_amd import decode_heads as dh
    gc.collect()
    gc.disable()
    try:
        head = dh.DAFormerHead(**dict(TS.HEAD_KW, sampler=dict(SAMPLER)), decoder_params=TS.decoder_params())
        twin = copy.deepcopy(head)
        assert twin.sampler is not head.sampler and twin.sampler.context is twin and head.sampler.context is head
        assert (twin.sampler.thresh, twin.sampler.min_kept) == (0.7, 64)
        ref = weakref.ref(head)
        del head
        assert ref() is None, 'the head is part of a reference cycle'
    finally:
        gc.enable()


# ---------------------------------------------------------------------------------------------------------------------------
# one DACS iteration, eager and as a replayed graph
def _dacs_run(dev, sampler, graph, iters=2):
    cfg = TD.make_cfg(**TD.SMALL, generator=False)
    if sampler is not None:
        cfg['model']['decode_head']['sampler'] = dict(sampler)
    dacs = build_train_model(cfg)
    seeded_fill(dacs.model, 7)
    seeded_fill(dacs.ema_model, 8)
    with torch.no_grad():   # logits of a scale at which some pixels are confident: at the seeded scale every pixel is hard
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    dacs.to(dev).train()
    src, tg = TD.make_batch(2, 64, 64)
    batch = dict(source={k: v.to(dev) for k, v in src.items()}, target={k: v.to(dev) for k, v in tg.items()})
    torch.manual_seed(11), random.seed(11), np.random.seed(11)
    if graph:
        dacs.enable_graph(warmup_iters=1)
    out = []
    for it in range(iters):
        for p in dacs.model.parameters():
            if p.grad is not None:
                p.grad.zero_()
        lv = dacs(**batch)
        torch.cuda.synchronize()
        out.append({k: float(v) for k, v in lv.items() if 'loss' in k})
    if graph:
        assert dacs._graph is not None, 'the iteration was not captured'
    return out


@pytest.mark.gpu
def test_dacs_iteration_with_sampler_eager_and_captured_gpu():
    """the smallest configuration of tests/test_dacs.py with the sampler in the decode head: two iterations eager against warm-up +
    hipGraph replay (the sampler has no host synchronisation, so the captured iteration holds it).  The losses agree to the bound of
    the other graph-against-eager tests (1e-4: the cross-entropy sum and the BatchNorm statistics add fp32 partials with atomics, in
    an order that is free from run to run), and the sampler moves decode.loss_seg."""
    dev = TS._gpu().device
    rt.set_compute_dtype(torch.float32)
    sampler = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=64)
    eager, captured, plain = _dacs_run(dev, sampler, False), _dacs_run(dev, sampler, True), _dacs_run(dev, None, False, iters=1)
    for it, (l_e, l_g) in enumerate(zip(eager, captured)):
        assert l_e.keys() == l_g.keys() and 'decode.loss_seg' in l_e and 'mix.decode.loss_seg' in l_e
        assert all(np.isfinite(v) for v in l_e.values()) and all(np.isfinite(v) for v in l_g.values())
        for k in l_e:
            assert_close(torch.tensor([l_g[k]]), torch.tensor([l_e[k]]), 1e-4, name=f'it{it} {k}, graph vs eager, with the sampler')
    # the source loss loses its confident, correct pixels (a few of 8192 for this model: 15.1466 against 15.1530 on the emulator); the
    # mixed loss also loses DACS's pseudo-weight, the confident share of the teacher's pixels, so it grows by a large factor
    print('decode.loss_seg', eager[0]['decode.loss_seg'], 'without the sampler', plain[0]['decode.loss_seg'],
          '; mix.decode.loss_seg', eager[0]['mix.decode.loss_seg'], 'without', plain[0]['mix.decode.loss_seg'])
    # "differs": by more than two runs of the SAME computation may (the 1e-4 of the agreement check above)
    check_ge('decode.loss_seg moved by the sampler, relative', abs(eager[0]['decode.loss_seg'] - plain[0]['decode.loss_seg']) / plain[0]['decode.loss_seg'],
             1e-4, strict=True)
    check_ge('mix.decode.loss_seg moved by the sampler, relative',
             abs(eager[0]['mix.decode.loss_seg'] - plain[0]['mix.decode.loss_seg']) / plain[0]['mix.decode.loss_seg'], 1e-2)


if __name__ == '__main__':
    d = _reference_fp32_distance()
    print('REF_DIST = {' + ', '.join(f'{k!r}: ({v[0]:.3e}, {v[1]:.3e})' for k, v in d.items()) + '}')
