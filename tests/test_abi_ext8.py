"""The eighth ABI extension (include/cmda_hip_ext8.h, prefix `cmdax8_`): the guarantees tests/test_abi_ext7.py gives the seventh one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext8.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax8_\w+)\(', text)))


def test_eighth_table_symbols_exported_by_hip_library():
    from cmda_amd._lib import Level8
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax8_abi_version', 'cmdax8_bn_stats', 'cmdax8_resavg_bwd', 'cmdax8_resavg_fwd', 'cmdax8_ws_floats']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext8.h but not exported'
    assert lib.cmdax8_abi_version() == 1
    # the frozen tables do not move
    assert lib.cmdax7_abi_version() == 1 and lib.cmdax6_abi_version() == 1 and lib.cmdax5_abi_version() == 1
    assert lib.cmdax4_abi_version() == 1 and lib.cmdax3_abi_version() == 1
    assert lib.cmdax2_abi_version() == 1 and lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8
    # the descriptor the binding fills is the header's: 2 x 10 pointers, 2 pointers, int64, 2 x int32
    assert ctypes.sizeof(Level8) == 2 * 10 * 8 + 2 * 8 + 8 + 2 * 4
    # the workspace query and the refusals are decided before any HIP call: they can be asked for without a GPU
    i32, i64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    lib.cmdax8_ws_floats.restype = ctypes.c_int64
    lib.cmdax8_ws_floats.argtypes = [vp, ctypes.c_int, ctypes.c_int]

    def levels(n=1, C=64, M=16, fake=64):
        arr = (Level8 * n)()
        for d in arr:
            d.M, d.C, d.out, d.dout = M, C, fake, fake
            for b in d.br:
                for name, _ in b._fields_:
                    setattr(b, name, fake)
        return arr
    assert lib.cmdax8_ws_floats(levels(), 1, 1) == 2 * 33 * 2 * 64
    four = levels(4)
    for d, c in zip(four, (64, 128, 320, 512)):
        d.C = c
    assert lib.cmdax8_ws_floats(four, 4, 2) == 2 * 2 * 33 * 2 * (64 + 128 + 320 + 512)
    assert lib.cmdax8_ws_floats(levels(C=6), 1, 1) == -1 and lib.cmdax8_ws_floats(levels(), 0, 1) == -1
    assert lib.cmdax8_ws_floats(levels(), 5, 1) == -1 and lib.cmdax8_ws_floats(levels(), 1, 0) == -1
    assert lib.cmdax8_ws_floats(levels(), 1, 9) == -1 and lib.cmdax8_ws_floats(None, 1, 1) == -1

    def fwd(arr, n=1, groups=1, dtype=0):
        return lib.cmdax8_resavg_fwd(arr, i32(n), i32(groups), i32(dtype), None)

    def bwd(arr, n=1, groups=1, dtype=0, ws=vp(64)):
        return lib.cmdax8_resavg_bwd(arr, i32(n), i32(groups), ws, i32(dtype), None)
    for call in (fwd, bwd):   # (the fake pointers are never dereferenced: every call below is refused on the host)
        assert call(levels(C=6)) == -1 and call(levels(C=0)) == -1 and call(levels(M=0)) == -1
        assert call(levels(), n=0) == -1 and call(levels(), n=5) == -1 and call(levels(), groups=0) == -1 and call(levels(), groups=9) == -1
        assert call(levels(C=64, M=2 ** 31 // 64)) == -1 and call(levels(C=64, M=2 ** 31 // 128), groups=2) == -1
        assert call(levels(), dtype=2) == -2 and call(levels(C=6), dtype=2) == -1
        assert call(None) == -4
        arr = levels()
        arr[0].br[1].rstd = None
        assert call(arr) == -4
    arr = levels()
    arr[0].out = None
    assert fwd(arr) == -4
    for name in ('dz', 'dres', 'dgamma', 'dbeta'):
        arr = levels()
        setattr(arr[0].br[0], name, None)
        assert bwd(arr) == -4, name
    arr = levels()
    arr[0].dout = None
    assert bwd(arr) == -4 and bwd(levels(), ws=None) == -4

    def stats(C=8, groups=1, order=None, has=0, dtype=0):
        oc = (ctypes.c_int * len(order))(*order) if order else None
        return lib.cmdax8_bn_stats(vp(64), vp(64), vp(64), None, None, vp(64), i64(4), i32(C), f32(1e-5), f32(0.1), i32(groups), oc,
                                   i32(has), i32(dtype), None)
    assert stats(C=6) == -1 and stats(groups=0) == -1 and stats(groups=9) == -1 and stats(groups=2, order=(0, 2)) == -1
    assert stats(groups=2, order=(1, 1), has=1) == -1 and stats(dtype=3) == -2


def test_every_exported_eighth_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax8_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_eighth_header_is_a_build_dependency():
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, re.M).group(1)
    assert 'include/cmda_hip_ext8.h' in hdrs.split()


def test_binding_checks_the_eighth_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT8_VERSION == 1
    earlier = ('cmdax_abi_version', 'cmdax2_abi_version', 'cmdax3_abi_version', 'cmdax4_abi_version', 'cmdax5_abi_version',
               'cmdax6_abi_version', 'cmdax7_abi_version')

    class Old:   # a library from before the eighth table: the earlier ones are there and current
        def __getattr__(self, name):
            if name.startswith('cmdax8_'):
                raise AttributeError(name)
            return lambda *a: 1 if name in earlier else 0
    old = Old()
    assert _lib._declare(old) is old   # `_declare` ends with the seventh table ...
    try:
        _lib._declare_ext8(old)          # ... the eighth is checked by the function `_load` / `_bind_for_tests` call right behind it
    except _lib.CmdaError as e:
        assert 'cmdax8_' in str(e) and 'lacks the eighth ABI table' in str(e)
    else:
        raise AssertionError('a library without the eighth table must be rejected')

    class Stale(Old):   # the eighth table is there, at another version
        def __getattr__(self, name):
            if name == 'cmdax8_abi_version':
                return lambda *a: 2
            if name.startswith('cmdax8_'):
                return lambda *a: 0
            return Old.__getattr__(self, name)
    try:
        _lib._declare_ext8(_lib._declare(Stale()))
    except _lib.CmdaError as e:
        assert 'cmdax8_' in str(e) and 'version' in str(e)
    else:
        raise AssertionError('an eighth table of another version must be rejected')

    class Current(Old):   # every table there and current: accepted
        def __getattr__(self, name):
            if name == 'cmdax8_abi_version':
                return lambda *a: 1
            if name.startswith('cmdax8_'):
                return type('Fn', (), {'__call__': lambda self, *a: 0})()
            return Old.__getattr__(self, name)
    lib = Current()
    assert _lib._declare_ext8(_lib._declare(lib)) is lib

    class Seventh:   # the stand-in of tests/test_abi_ext7.py (0 for every name it does not know): `_declare` alone still accepts it
        def __getattr__(self, name):
            if name == 'cmdax7_abi_version':
                return lambda *a: 1
            return lambda *a: 1 if name in earlier else 0
    s = Seventh()
    assert _lib._declare(s) is s
    # both loaders run the check: their source calls it on what `_declare` returns
    import inspect
    for fn in (_lib._load, _lib._bind_for_tests):
        assert '_declare_ext8(_declare(' in inspect.getsource(fn), fn.__name__


_T = 'test_resblock.py'
KERNEL_TESTS = {
    'cmdax8_abi_version': ['test_abi_ext8.py::test_eighth_table_symbols_exported_by_hip_library'],
    'cmdax8_ws_floats': ['test_abi_ext8.py::test_eighth_table_symbols_exported_by_hip_library', f'{_T}::test_eighth_table_refusals'],
    'cmdax8_resavg_fwd': [f'{_T}::test_resavg_against_float64', f'{_T}::test_resavg_four_levels_one_grid',
                          f'{_T}::test_resavg_groups_use_their_own_statistics', f'{_T}::test_eighth_table_refusals'],
    'cmdax8_resavg_bwd': [f'{_T}::test_resavg_against_float64', f'{_T}::test_resavg_four_levels_one_grid', f'{_T}::test_eighth_table_refusals'],
    'cmdax8_bn_stats': [f'{_T}::test_bn_stats', f'{_T}::test_eighth_table_refusals'],
}


def test_every_eighth_table_entry_point_has_a_kernel_level_test():
    declared = set(declared_symbols())
    assert set(KERNEL_TESTS) == declared, f'untested: {sorted(declared - set(KERNEL_TESTS))}, gone: {sorted(set(KERNEL_TESTS) - declared)}'
    here = os.path.dirname(os.path.abspath(__file__))
    defs = {}
    for sym, tests in KERNEL_TESTS.items():
        for t in tests:
            fname, func = t.split('::')
            if fname not in defs:
                defs[fname] = set(re.findall(r'^def (test_\w+)\(', open(os.path.join(here, fname)).read(), re.M))
            assert func in defs[fname], f'{sym}: {t} does not exist'
