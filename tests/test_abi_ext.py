"""The ABI extension (include/cmda_hip_ext.h, prefix `cmdax_`): the guarantees tests/test_abi.py gives the frozen core table
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext.h')).read()
    return sorted(set(re.findall(r'\bint (cmdax_\w+)\(', text)))


def test_extension_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert len(syms) >= 3
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext.h but not exported'
    assert lib.cmdax_abi_version() == 1
    assert lib.cmda_abi_version() == 8          # the core table is frozen: the extension does not move its version


def test_every_exported_extension_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" int (cmdax_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_binding_checks_the_extension_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT_VERSION == 1

    class Old:   # a library from before the extension
        def __getattr__(self, name):
            if name.startswith('cmdax_'):
                raise AttributeError(name)
            return lambda *a: 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'extension' in str(e)
    else:
        raise AssertionError('a library without the extension table must be rejected')


_S = 'test_seg_eval.py'
KERNEL_TESTS = {
    'cmdax_abi_version': ['test_abi_ext.py::test_extension_symbols_exported_by_hip_library'],
    'cmdax_confusion_update': [f'{_S}::test_confusion_matches_reference_golden', f'{_S}::test_fused_score_equals_two_step',
                               f'{_S}::test_seg_eval_refusals'],
    'cmdax_seg_predict': [f'{_S}::test_seg_predict_matches_torch', f'{_S}::test_seg_predict_equals_existing_path',
                          f'{_S}::test_fused_score_equals_two_step', f'{_S}::test_seg_eval_refusals'],
}


def test_every_extension_entry_point_has_a_kernel_level_test():
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
