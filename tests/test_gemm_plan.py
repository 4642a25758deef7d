"""cmda_gemm's dispatch plan (csrc/gemm.hip plan_gemm, queried through cmda_debug_gemm_plan): which kernel family, tile, LDS stages,
waves and split count a parameter block gets.  Host only: no launch, no GPU, operand pointers are fake aligned addresses.

EXPECTED was recorded from the commit BEFORE the plan existed: its emulator library with a log line in every launcher (family, tile /
stage / wave template arguments, split count) and the launches skipped, run over exactly these parameter blocks.  The two cases the
plan deliberately changes are asserted on their own below."""
import ast
import ctypes
import os
import re
import subprocess

import pytest

from cmda_amd._lib import GemmParams, View

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED = 0, -4
NONE, PINGPONG, WGRAD, GLDS, LEAN, REG, X3REG, X3LEAN = range(8)   # GemmFamily
T128, T128x64, T64, T256 = range(4)                                  # GemmTile
F32, BF16, F32X3 = 0, 1, 2


def _library():
    for rel in ('cmda_amd/libcmda_hip.so', 'tests/emu/libcmda_emu.so'):
        if os.path.exists(os.path.join(ROOT, rel)):
            return ctypes.CDLL(os.path.join(ROOT, rel))   # loads without a GPU: no HIP call happens at load time
    subprocess.check_call(['make', '-j8', 'emu'], cwd=ROOT, stdout=subprocess.DEVNULL)
    return ctypes.CDLL(os.path.join(ROOT, 'tests/emu/libcmda_emu.so'))


def plan(p, lib=[]):
    if not lib:
        lib.append(_library())
    out = (ctypes.c_int32 * 7)()
    assert lib[0].cmda_debug_gemm_plan(ctypes.byref(p), out) == 0
    return tuple(out)[:6] if out[0] == OK else (out[0], out[1])


def plain(rows, cols, ptr, es):
    return View(ptr=ptr, ld=cols, R=rows, Cc=cols, conv=0, vec_ok=int(cols % (16 // es) == 0), H=0, W=0, C=1, OH=1, OW=1, KH=1, KW=1,
                stride=1, pad=0, dil=1, in_dil=1, reflect=0)


def im2col(B, H, W, C, k, pad, ptr):   # stride-1 "same" convolution
    return View(ptr=ptr, ld=0, R=B * H * W, Cc=k * k * C, conv=1, vec_ok=1, H=H, W=W, C=C, OH=H, OW=W, KH=k, KW=k, stride=1, pad=pad,
                dil=1, in_dil=1, reflect=0)


def problem(M, N, K, aks=0, bks=0, atomic=0, dtype=BF16, hint=0, B=None, **kw):
    """the blocks tools/gemm_sweep.py issues: plain operands, fp32 atomics with the library's split count or a plain bf16 / fp32 store"""
    es = 2 if dtype == BF16 else 4
    p = GemmParams()
    p.A = plain(K, M, 0x10000, es) if aks else plain(M, K, 0x10000, es)
    p.B = B if B is not None else plain(K, N, 0x20000, es) if bks else plain(N, K, 0x20000, es)
    p.a_kstrided, p.b_kstrided, p.C, p.ldc = aks, bks, 0x30000, N
    p.M, p.N, p.K, p.batch, p.batch2, p.splits = M, N, K, 1, 1, 0 if atomic else 1
    p.alpha, p.rows_per_scale, p.dtype, p.c_vec_ok, p.tile_hint = 1.0, 1, dtype, 1, hint
    p.atomic, p.out_f32 = atomic, int(bool(atomic) or dtype != BF16)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def sweep_shapes():
    text = open(os.path.join(ROOT, 'tools', 'gemm_sweep.py')).read()
    shapes = ast.literal_eval(re.search(r'^SHAPES = (\[.*?^\])', text, re.M | re.S).group(1))
    assert len(shapes) == 33
    return shapes


def cases():
    c = {}
    for M, N, K, aks, bks, atomic in sweep_shapes():
        c[f'bf16 {M}x{N}x{K} aks{aks} bks{bks} atomic{atomic}'] = problem(M, N, K, aks, bks, atomic)
        c[f'x3 {M}x{N}x{K} forward'] = problem(M, N, K, dtype=F32X3)
    # the large shapes the comments of gemm.hip name
    c['bf16 8192^3 NT'] = problem(8192, 8192, 8192)
    c['bf16 8192^3 NN'] = problem(8192, 8192, 8192, bks=1)
    c['bf16 65536x1280x320'] = problem(65536, 1280, 320)
    c['bf16 262144x1024x256'] = problem(262144, 1024, 256)
    c['bf16 wgrad 256x1024 over 262144'] = problem(256, 1024, 262144, 1, 1, 1)
    c['bf16 wgrad 1024x256 over 262144'] = problem(1024, 256, 262144, 1, 1, 1)
    c['bf16 wgrad 3x3 bottleneck 256x9216 over 262144'] = problem(256, 9216, 262144, 1, 1, 1, B=im2col(16, 128, 128, 1024, 3, 1, 0x20000),
                                                                  c_perm_ci=1024, c_perm_cells=9)
    # refusals
    c['bf16 colsum, A K-contiguous'] = problem(2048, 320, 320, colsum=0x40000)
    # the hints the suite uses
    for hint in (1, 2, 3, 4, -1):
        c[f'bf16 2048x320x320 hint {hint}'] = problem(2048, 320, 320, hint=hint)
    for hint in (516, 1028):
        c[f'bf16 1024x512x512 hint {hint}'] = problem(1024, 512, 512, hint=hint)
    c['bf16 2048x320x1280 hint 8192'] = problem(2048, 320, 1280, hint=8192)
    c['bf16 64x64x256 hint 3'] = problem(64, 64, 256, hint=3)
    c['bf16 600x1100x256 hint 3|256'] = problem(600, 1100, 256, hint=3 | 256)
    for hint in (8192, 65536):
        c[f'x3 16384x512x128 hint {hint}'] = problem(16384, 512, 128, dtype=F32X3, hint=hint)
    c['x3 wgrad 320x1280 over 8192 hint 65536'] = problem(320, 1280, 8192, 1, 1, 1, dtype=F32X3, hint=65536)
    return c


# case -> (return code, family, tile, LDS stages, waves, splits); refusals: (return code, NONE)
EXPECTED = {
    'bf16 2048x320x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 2048x320x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 4096x320x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 4096x320x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 8192x320x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 8192x320x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 2048x1280x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 2048x1280x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 4096x1280x320 aks0 bks0 atomic0': (OK, LEAN, T128x64, 2, 8, 1),
    'x3 4096x1280x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 8192x1280x320 aks0 bks0 atomic0': (OK, LEAN, T128x64, 2, 8, 1),
    'x3 8192x1280x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 2048x320x1280 aks0 bks0 atomic0': (OK, LEAN, T64, 4, 4, 1),
    'x3 2048x320x1280 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 4096x320x1280 aks0 bks0 atomic0': (OK, LEAN, T64, 4, 4, 1),
    'x3 4096x320x1280 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 8192x320x1280 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 8192x320x1280 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 4096x320x1280 aks0 bks1 atomic0': (OK, LEAN, T64, 4, 4, 1),
    'bf16 8192x320x1280 aks0 bks1 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'bf16 4096x1280x320 aks0 bks1 atomic0': (OK, LEAN, T128x64, 2, 8, 1),
    'bf16 8192x1280x320 aks0 bks1 atomic0': (OK, LEAN, T128x64, 2, 8, 1),
    'bf16 4096x320x320 aks0 bks1 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'bf16 8192x320x320 aks0 bks1 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'bf16 512x640x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 512x640x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 1024x640x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 1024x640x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 2048x640x320 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 2048x640x320 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 320x1280x8192 aks1 bks1 atomic1': (OK, GLDS, T64, 2, 4, 6),
    'x3 320x1280x8192 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 320x320x8192 aks1 bks1 atomic1': (OK, GLDS, T64, 2, 4, 16),
    'x3 320x320x8192 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 1280x320x8192 aks1 bks1 atomic1': (OK, GLDS, T64, 2, 4, 6),
    'x3 1280x320x8192 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 320x320x4096 aks1 bks1 atomic1': (OK, GLDS, T64, 2, 4, 8),
    'x3 320x320x4096 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 1280x320x4096 aks1 bks1 atomic1': (OK, GLDS, T64, 2, 4, 6),
    'x3 1280x320x4096 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 640x320x2048 aks1 bks1 atomic1': (OK, GLDS, T64, 2, 4, 4),
    'x3 640x320x2048 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 16384x128x128 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 16384x128x128 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 16384x512x128 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 16384x512x128 forward': (OK, X3REG, T128, 0, 4, 1),
    'bf16 16384x128x512 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 16384x128x512 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 65536x64x64 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 65536x64x64 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 65536x256x64 aks0 bks0 atomic0': (OK, PINGPONG, T256, 0, 8, 1),
    'x3 65536x256x64 forward': (OK, X3REG, T128, 0, 4, 1),
    'bf16 65536x64x256 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 65536x64x256 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 1024x512x512 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 1024x512x512 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 1024x2048x512 aks0 bks0 atomic0': (OK, LEAN, T64, 2, 8, 1),
    'x3 1024x2048x512 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 1024x512x2048 aks0 bks0 atomic0': (OK, LEAN, T64, 4, 4, 1),
    'x3 1024x512x2048 forward': (OK, X3LEAN, T64, 0, 8, 1),
    'bf16 8192^3 NT': (OK, GLDS, T256, 2, 8, 1),
    'bf16 8192^3 NN': (OK, PINGPONG, T256, 0, 8, 1),
    'bf16 65536x1280x320': (OK, PINGPONG, T256, 0, 8, 1),
    'bf16 262144x1024x256': (OK, PINGPONG, T256, 0, 8, 1),
    'bf16 wgrad 256x1024 over 262144': (OK, WGRAD, T256, 0, 8, 61),
    'bf16 wgrad 1024x256 over 262144': (OK, WGRAD, T256, 0, 8, 61),
    'bf16 wgrad 3x3 bottleneck 256x9216 over 262144': (OK, WGRAD, T256, 0, 8, 7),
    'bf16 colsum, A K-contiguous': (UNSUPPORTED, NONE),
    'bf16 2048x320x320 hint 1': (OK, GLDS, T128, 2, 4, 1),
    'bf16 2048x320x320 hint 2': (OK, LEAN, T128x64, 2, 8, 1),
    'bf16 2048x320x320 hint 3': (OK, LEAN, T64, 2, 8, 1),
    'bf16 2048x320x320 hint 4': (OK, PINGPONG, T256, 0, 8, 1),
    'bf16 2048x320x320 hint -1': (OK, REG, T64, 0, 4, 1),
    'bf16 1024x512x512 hint 516': (OK, GLDS, T256, 2, 8, 1),
    'bf16 1024x512x512 hint 1028': (OK, PINGPONG, T256, 0, 8, 1),
    'bf16 2048x320x1280 hint 8192': (OK, GLDS, T64, 4, 4, 1),
    'bf16 64x64x256 hint 3': (OK, LEAN, T64, 2, 8, 1),
    'bf16 600x1100x256 hint 3|256': (OK, LEAN, T64, 2, 8, 1),
    'x3 16384x512x128 hint 8192': (OK, X3REG, T128, 0, 4, 1),
    'x3 16384x512x128 hint 65536': (OK, X3LEAN, T64, 0, 8, 1),
    'x3 wgrad 320x1280 over 8192 hint 65536': (OK, X3LEAN, T64, 0, 8, 9),
}


CASES = cases()


def test_every_case_has_a_recorded_plan():
    assert set(CASES) == set(EXPECTED)


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_plan_matches_recorded_dispatch(name):
    assert plan(CASES[name]) == EXPECTED[name]


def test_hint_fields_do_not_collide():
    """bit 13 (general kernel instead of the lean one) used to be read a second time as a minimum k-tile count of 2 for the four-stage
    configuration: four k-tiles on a resident grid ran on four stages.  The switch now changes the kernel only."""
    assert plan(problem(64, 64, 256, hint=8192 | 3)) == (OK, GLDS, T64, 2, 4, 1)


@pytest.mark.parametrize('hint', [4096, 16384, 32768, 1 << 17, 3 | (12 << 12)])
def test_unknown_hint_bits_are_refused(hint):
    assert plan(problem(2048, 320, 320, hint=hint)) == (UNSUPPORTED, NONE)
