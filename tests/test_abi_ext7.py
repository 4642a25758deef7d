"""The seventh ABI extension (include/cmda_hip_ext7.h, prefix `cmdax7_`): the guarantees tests/test_abi_ext6.py gives the sixth one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext7.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax7_\w+)\(', text)))


def test_seventh_table_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax7_abi_version', 'cmdax7_ohem_weight', 'cmdax7_select_kth', 'cmdax7_ws_bytes']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext7.h but not exported'
    assert lib.cmdax7_abi_version() == 1
    # the frozen tables do not move
    assert lib.cmdax6_abi_version() == 1 and lib.cmdax5_abi_version() == 1 and lib.cmdax4_abi_version() == 1 and lib.cmdax3_abi_version() == 1
    assert lib.cmdax2_abi_version() == 1 and lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8
    # the workspace query and the refusals are decided before any HIP call: they can be asked for without a GPU
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.cmdax7_ws_bytes.restype = ctypes.c_int64
    lib.cmdax7_ws_bytes.argtypes = [ctypes.c_int64]
    counters = lib.cmdax7_ws_bytes(0)
    assert counters >= 4 * (2048 + 2048 + 1024 + 1) and counters % 16 == 0
    assert lib.cmdax7_ws_bytes(2 * 512 * 512) == counters + 4 * 2 * 512 * 512
    assert lib.cmdax7_ws_bytes(-1) == -1 and lib.cmdax7_ws_bytes(1 << 31) == -1 and lib.cmdax7_ws_bytes((1 << 31) - 1) > 0

    def ohem(nc=19, mode=0, min_kept=2, fake=None):
        return lib.cmdax7_ohem_weight(fake, fake, fake, None, fake, i32(1), i32(2), i32(2), i32(8), i32(8), i32(nc), i32(255), i32(mode),
                                      f32(0.7), i32(min_kept), None)
    assert ohem(nc=33) == -1 and ohem(nc=0) == -1 and ohem(min_kept=1) == -1
    assert ohem() == -4
    fake = ctypes.c_void_p(64)   # never dereferenced: the mode is refused on the host
    assert ohem(mode=2, fake=fake) == -4 and ohem(mode=2, min_kept=1, fake=fake) == -1
    assert lib.cmdax7_select_kth(None, i64(0), None, None, None, None) == -1
    assert lib.cmdax7_select_kth(None, i64(1 << 31), None, None, None, None) == -1
    assert lib.cmdax7_select_kth(None, i64(16), None, None, None, None) == -4


def test_every_exported_seventh_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax7_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_seventh_header_is_a_build_dependency():
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, re.M).group(1)
    assert 'include/cmda_hip_ext7.h' in hdrs.split()


def test_binding_checks_the_seventh_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT7_VERSION == 1
    earlier = ('cmdax_abi_version', 'cmdax2_abi_version', 'cmdax3_abi_version', 'cmdax4_abi_version', 'cmdax5_abi_version',
               'cmdax6_abi_version')

    class Old:   # a library from before the seventh table: the earlier ones are there and current
        def __getattr__(self, name):
            if name.startswith('cmdax7_'):
                raise AttributeError(name)
            return lambda *a: 1 if name in earlier else 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'cmdax7_' in str(e)
    else:
        raise AssertionError('a library without the seventh table must be rejected')

    class Stale(Old):   # the seventh table is there, at another version
        def __getattr__(self, name):
            if name == 'cmdax7_abi_version':
                return lambda *a: 2
            if name.startswith('cmdax7_'):
                return lambda *a: 0
            return Old.__getattr__(self, name)
    try:
        _lib._declare(Stale())
    except _lib.CmdaError as e:
        assert 'cmdax7_' in str(e) and 'version' in str(e)
    else:
        raise AssertionError('a seventh table of another version must be rejected')

    class NoSixth(Old):   # the sixth table's check comes first: its message is the one an older library gets
        def __getattr__(self, name):
            if name.startswith('cmdax6_'):
                raise AttributeError(name)
            return Old.__getattr__(self, name)
    try:
        _lib._declare(NoSixth())
    except _lib.CmdaError as e:
        assert 'cmdax6_' in str(e)
    else:
        raise AssertionError('a library without the sixth table must be rejected')

    class Current(Old):   # every table there and current: accepted
        def __getattr__(self, name):
            if name == 'cmdax7_abi_version':
                return lambda *a: 1
            if name.startswith('cmdax7_'):
                return lambda *a: 0
            return Old.__getattr__(self, name)
    lib = Current()
    assert _lib._declare(lib) is lib


_T = 'test_ohem.py'
KERNEL_TESTS = {
    'cmdax7_abi_version': ['test_abi_ext7.py::test_seventh_table_symbols_exported_by_hip_library'],
    'cmdax7_ws_bytes': ['test_abi_ext7.py::test_seventh_table_symbols_exported_by_hip_library', f'{_T}::test_seventh_table_refusals'],
    'cmdax7_select_kth': [f'{_T}::test_select_kth_is_exact', f'{_T}::test_select_kth_any_shape_and_clamped_k', f'{_T}::test_seventh_table_refusals'],
    'cmdax7_ohem_weight': [f'{_T}::test_ohem_weight_matches_float64_restatement', f'{_T}::test_ohem_weight_matches_reference_sampler',
                           f'{_T}::test_ohem_every_label_ignored', f'{_T}::test_ohem_one_valid_pixel',
                           f'{_T}::test_ohem_out_of_range_labels_are_invalid', f'{_T}::test_ohem_loss_mode_takes_every_tie_at_the_boundary',
                           f'{_T}::test_seventh_table_refusals'],
}


def test_every_seventh_table_entry_point_has_a_kernel_level_test():
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
