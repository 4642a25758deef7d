"""The fourth ABI extension (include/cmda_hip_ext4.h, prefix `cmdax4_`): the guarantees tests/test_abi_ext3.py gives the third one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext4.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax4_\w+)\(', text)))


def test_fourth_table_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax4_abi_version', 'cmdax4_cow_field', 'cmdax4_cow_mask', 'cmdax4_cow_mask_ws_bytes', 'cmdax4_isr_multi']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext4.h but not exported'
    assert lib.cmdax4_abi_version() == 1
    # the frozen tables do not move
    assert lib.cmdax3_abi_version() == 1 and lib.cmdax2_abi_version() == 1 and lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8
    lib.cmdax4_cow_mask_ws_bytes.restype = ctypes.c_int64
    B, H, W, K = 2, 100, 132, 195   # per sample: a pair of doubles per 32 x 32 tile, then two fp32 planes
    assert lib.cmdax4_cow_mask_ws_bytes(B, H, W, K) == 16 * B * ((H + 31) // 32) * ((W + 31) // 32) + 8 * B * H * W
    assert lib.cmdax4_cow_mask_ws_bytes(B, 33, 70, 9) == 16 * B * 2 * 3 + 8 * B * 33 * 70
    for bad in ((B, H, W, 194), (B, H, W, 257), (B, 97, W, 195), (B, H, 97, 195), (-1, H, W, K), (B, 0, W, 9)):
        assert lib.cmdax4_cow_mask_ws_bytes(*bad) == 0, f'{bad} is not a legal cow-mask shape'


def test_every_exported_fourth_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax4_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_binding_checks_the_fourth_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT4_VERSION == 1

    class Old:   # a library from before the fourth table: the earlier ones are there and current
        def __getattr__(self, name):
            if name.startswith('cmdax4_'):
                raise AttributeError(name)
            return lambda *a: 1 if name in ('cmdax_abi_version', 'cmdax2_abi_version', 'cmdax3_abi_version') else 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'cmdax4_' in str(e)
    else:
        raise AssertionError('a library without the fourth table must be rejected')


_M, _C = 'test_isr_multi.py', 'test_cow_mask.py'
KERNEL_TESTS = {
    'cmdax4_abi_version': ['test_abi_ext4.py::test_fourth_table_symbols_exported_by_hip_library'],
    'cmdax4_cow_mask_ws_bytes': ['test_abi_ext4.py::test_fourth_table_symbols_exported_by_hip_library',
                                 f'{_C}::test_cow_mask_last_legal_padding'],
    'cmdax4_isr_multi': [f'{_M}::test_isr_multi_reproduces_the_reference_presets', f'{_M}::test_isr_multi_is_bit_identical_to_isr_from_gray',
                         f'{_M}::test_isr_multi_flat_image', f'{_M}::test_isr_multi_window', f'{_M}::test_isr_multi_refusals'],
    'cmdax4_cow_mask': [f'{_C}::test_cow_mask_reproduces_the_reference', f'{_C}::test_cow_mask_last_legal_padding',
                        f'{_C}::test_cow_mask_small_kernel', f'{_C}::test_cow_mask_generated_field', f'{_C}::test_cow_mask_refusals'],
    'cmdax4_cow_field': [f'{_C}::test_cow_mask_generated_field', f'{_C}::test_cow_field_statistics', f'{_C}::test_cow_mask_refusals'],
}


def test_every_fourth_table_entry_point_has_a_kernel_level_test():
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
