"""The sixth ABI extension (include/cmda_hip_ext6.h, prefix `cmdax6_`): the guarantees tests/test_abi_ext5.py gives the fifth one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext6.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax6_\w+)\(', text)))


def test_sixth_table_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax6_abi_version', 'cmdax6_split_targets', 'cmdax6_split_weights']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext6.h but not exported'
    assert lib.cmdax6_abi_version() == 1
    # the frozen tables do not move
    assert lib.cmdax5_abi_version() == 1 and lib.cmdax4_abi_version() == 1 and lib.cmdax3_abi_version() == 1
    assert lib.cmdax2_abi_version() == 1 and lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8
    # refusals are decided before any HIP call: they can be asked for without a GPU
    i32 = ctypes.c_int32
    assert lib.cmdax6_split_targets(None, None, None, None, None, None, None, i32(1), i32(2), i32(2), i32(8), i32(8), i32(33), i32(10),
                                    ctypes.c_float(0.968), None) == -1
    assert lib.cmdax6_split_targets(None, None, None, None, None, None, None, i32(1), i32(2), i32(2), i32(8), i32(8), i32(19), i32(10),
                                    ctypes.c_float(0.968), None) == -4
    assert lib.cmdax6_split_weights(None, None, None, None, i32(1), i32(8), i32(8), i32(0), i32(0), i32(0), None) == -1
    assert lib.cmdax6_split_weights(None, None, None, None, i32(1), i32(8), i32(8), i32(10), i32(0), i32(0), None) == -4


def test_every_exported_sixth_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax6_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_sixth_header_is_a_build_dependency():
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, re.M).group(1)
    assert 'include/cmda_hip_ext6.h' in hdrs.split()


def test_binding_checks_the_sixth_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT6_VERSION == 1
    earlier = ('cmdax_abi_version', 'cmdax2_abi_version', 'cmdax3_abi_version', 'cmdax4_abi_version', 'cmdax5_abi_version')

    class Old:   # a library from before the sixth table: the earlier ones are there and current
        def __getattr__(self, name):
            if name.startswith('cmdax6_'):
                raise AttributeError(name)
            return lambda *a: 1 if name in earlier else 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'cmdax6_' in str(e)
    else:
        raise AssertionError('a library without the sixth table must be rejected')

    class Stale(Old):   # the sixth table is there, at another version
        def __getattr__(self, name):
            if name == 'cmdax6_abi_version':
                return lambda *a: 2
            if name.startswith('cmdax6_'):
                return lambda *a: 0
            return Old.__getattr__(self, name)
    try:
        _lib._declare(Stale())
    except _lib.CmdaError as e:
        assert 'cmdax6_' in str(e) and 'version' in str(e)
    else:
        raise AssertionError('a sixth table of another version must be rejected')

    class NoFifth(Old):   # the fifth table's check comes first: its message is the one an older library gets
        def __getattr__(self, name):
            if name.startswith('cmdax5_'):
                raise AttributeError(name)
            return Old.__getattr__(self, name)
    try:
        _lib._declare(NoFifth())
    except _lib.CmdaError as e:
        assert 'cmdax5_' in str(e)
    else:
        raise AssertionError('a library without the fifth table must be rejected')


_T = 'test_split_targets.py'
KERNEL_TESTS = {
    'cmdax6_abi_version': ['test_abi_ext6.py::test_sixth_table_symbols_exported_by_hip_library'],
    'cmdax6_split_targets': [f'{_T}::test_split_targets_equal_composed_ops', f'{_T}::test_split_targets_identical_maps_give_identical_halves',
                             f'{_T}::test_split_targets_swapped_maps_swap_the_halves', f'{_T}::test_sixth_table_refusals'],
    'cmdax6_split_weights': [f'{_T}::test_split_targets_equal_composed_ops', f'{_T}::test_split_targets_swapped_maps_swap_the_halves',
                             f'{_T}::test_sixth_table_refusals'],
}


def test_every_sixth_table_entry_point_has_a_kernel_level_test():
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
