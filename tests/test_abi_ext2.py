"""The second ABI extension (include/cmda_hip_ext2.h, prefix `cmdax2_`): the guarantees tests/test_abi_ext.py gives the first one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext2.h')).read()
    return sorted(set(re.findall(r'\bint (cmdax2_\w+)\(', text)))


def test_second_table_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax2_abi_version', 'cmdax2_prob_predict', 'cmdax2_seg_scores']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext2.h but not exported'
    assert lib.cmdax2_abi_version() == 1
    assert lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8     # the earlier tables are frozen: theirs do not move


def test_every_exported_second_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" int (cmdax2_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_binding_checks_the_second_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT2_VERSION == 1

    class Old:   # a library from before the second table: the first extension is there and current
        def __getattr__(self, name):
            if name.startswith('cmdax2_'):
                raise AttributeError(name)
            return lambda *a: 1 if name == 'cmdax_abi_version' else 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'cmdax2_' in str(e)
    else:
        raise AssertionError('a library without the second table must be rejected')

    class Stale(Old):   # ... and one whose second table has another version
        def __getattr__(self, name):
            if name == 'cmdax2_abi_version':
                return lambda *a: 2
            return lambda *a: 1 if name == 'cmdax_abi_version' else 0
    try:
        _lib._declare(Stale())
    except _lib.CmdaError as e:
        assert 'cmdax2_' in str(e) and 'version' in str(e)
    else:
        raise AssertionError('a library with another version of the second table must be rejected')


_T = 'test_tta.py'
KERNEL_TESTS = {
    'cmdax2_abi_version': ['test_abi_ext2.py::test_second_table_symbols_exported_by_hip_library'],
    'cmdax2_seg_scores': [f'{_T}::test_windows_match_torch', f'{_T}::test_windows_equal_existing_path',
                          f'{_T}::test_single_window_equals_seg_predict', f'{_T}::test_prob_accumulate',
                          f'{_T}::test_windows_fused_score_equals_two_step', f'{_T}::test_tta_refusals'],
    'cmdax2_prob_predict': [f'{_T}::test_prob_predict', f'{_T}::test_tta_refusals'],
}


def test_every_second_table_entry_point_has_a_kernel_level_test():
    declared = set(declared_symbols())
    assert set(KERNEL_TESTS) == declared, f'untested: {sorted(declared - set(KERNEL_TESTS))}, gone: {sorted(set(KERNEL_TESTS) - declared)}'
    here = os.path.dirname(os.path.abspath(__file__))
    defs = {}
    for sym, tests in KERNEL_TESTS.items():
        assert tests, f'{sym}: no test listed'
        for t in tests:
            fname, func = t.split('::')
            if fname not in defs:
                defs[fname] = set(re.findall(r'^def (test_\w+)\(', open(os.path.join(here, fname)).read(), re.M))
            assert func in defs[fname], f'{sym}: {t} does not exist'
