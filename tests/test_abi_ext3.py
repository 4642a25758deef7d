"""The third ABI extension (include/cmda_hip_ext3.h, prefix `cmdax3_`): the guarantees tests/test_abi_ext2.py gives the second one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext3.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax3_\w+)\(', text)))


def test_third_table_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax3_abi_version', 'cmdax3_isr_noise', 'cmdax3_randn_fields', 'cmdax3_sky_mask', 'cmdax3_sky_mask_ws_bytes']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext3.h but not exported'
    assert lib.cmdax3_abi_version() == 1
    assert lib.cmdax2_abi_version() == 1 and lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8   # the frozen tables do not move
    lib.cmdax3_sky_mask_ws_bytes.restype = ctypes.c_int64
    B, H, W = 2, 44, 70   # 4 statistics + H row counts per sample (rounded up to 16 bytes), then 2 + 1 bytes per pixel
    assert lib.cmdax3_sky_mask_ws_bytes(B, H, W) == (B * 4 + B * H + 3) // 4 * 16 + 3 * B * H * W


def test_every_exported_third_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax3_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_binding_checks_the_third_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT3_VERSION == 1

    class Old:   # a library from before the third table: the earlier ones are there and current
        def __getattr__(self, name):
            if name.startswith('cmdax3_'):
                raise AttributeError(name)
            return lambda *a: 1 if name in ('cmdax_abi_version', 'cmdax2_abi_version') else 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'cmdax3_' in str(e)
    else:
        raise AssertionError('a library without the third table must be rejected')


_T, _U = 'test_isr_augment.py', 'test_isr_augment_uda.py'
KERNEL_TESTS = {
    'cmdax3_abi_version': ['test_abi_ext3.py::test_third_table_symbols_exported_by_hip_library'],
    'cmdax3_sky_mask_ws_bytes': ['test_abi_ext3.py::test_third_table_symbols_exported_by_hip_library'],
    'cmdax3_sky_mask': [f'{_T}::test_sky_mask', f'{_T}::test_sky_mask_from_unit_input', f'{_T}::test_sky_mask_gate_and_in_place',
                        f'{_T}::test_kernels_reproduce_the_reference_outputs', f'{_T}::test_isr_augment_refusals'],
    'cmdax3_isr_noise': [f'{_T}::test_isr_noise_explicit_fields', f'{_T}::test_isr_noise_generated_fields',
                         f'{_T}::test_kernels_reproduce_the_reference_outputs', f'{_T}::test_isr_augment_refusals'],
    'cmdax3_randn_fields': [f'{_T}::test_isr_noise_generated_fields', f'{_T}::test_randn_fields_statistics'],
}


def test_every_third_table_entry_point_has_a_kernel_level_test():
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
