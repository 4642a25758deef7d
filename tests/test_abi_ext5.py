"""The fifth ABI extension (include/cmda_hip_ext5.h, prefix `cmdax5_`): the guarantees tests/test_abi_ext4.py gives the fourth one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext5.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax5_\w+)\(', text)))


def voxel_ws_bytes(B, n_total, bins, H, W):
    """the formula of the header: offsets, (key, weight) records, per-cell counters + the long-cell counter, scan partials, long-cell list"""
    cells = B * bins * H * W
    total = 8 * (B + 1) + 4 * (cells + 2) + 4 * B * -(-(bins * H * W) // 2048) + 4 * (min(cells, 8 * n_total // 33) + 1) + 64 * n_total
    return -(-total // 8) * 8


def test_fifth_table_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax5_abi_version', 'cmdax5_event_prep_batch', 'cmdax5_events_norm_batch', 'cmdax5_events_norm_ws_bytes',
                    'cmdax5_voxel_ordered', 'cmdax5_voxel_ordered_ws_bytes']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext5.h but not exported'
    assert lib.cmdax5_abi_version() == 1
    # the frozen tables do not move
    assert lib.cmdax4_abi_version() == 1 and lib.cmdax3_abi_version() == 1 and lib.cmdax2_abi_version() == 1
    assert lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8
    ws = lib.cmdax5_voxel_ordered_ws_bytes
    ws.restype = ctypes.c_int64
    ws.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert ws(2, 1000000, 5, 480, 640) == voxel_ws_bytes(2, 1000000, 5, 480, 640)     # the step's shape: the record buffer dominates
    assert ws(3, 5779, 2, 12, 16) == voxel_ws_bytes(3, 5779, 2, 12, 16)               # fewer cells than possible long segments
    assert ws(1, 0, 1, 1, 1) == voxel_ws_bytes(1, 0, 1, 1, 1) == 40
    for bad in ((0, 10, 1, 4, 4), (257, 10, 1, 4, 4), (1, 10, 0, 4, 4), (1, 10, 1, 0, 4), (1, 10, 1, 4, -1), (1, -1, 1, 4, 4),
                (2, 10, 1 << 10, 1 << 10, 1 << 10), (1, 1 << 29, 1, 4, 4), (2, 1 << 30, 1, 4, 4)):
        assert ws(*bad) == 0, f'{bad} is not a legal ordered-voxel shape'
    assert ws(2, (1 << 30) - 2, 1, 4, 4) > 0   # two samples just below the per-sample limit
    nws = lib.cmdax5_events_norm_ws_bytes
    nws.restype = ctypes.c_int64
    nws.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert nws(2, 5 * 480 * 640) == 24 * 2 * 256 + 16 * 2      # capped at 256 partials
    assert nws(3, 5000) == 24 * 3 * 3 + 16 * 3                 # ceil(5000 / 2048) partials
    for bad in ((0, 100), (257, 100), (1, 0), (2, 1 << 30)):
        assert nws(*bad) == 0, f'{bad} is not a legal events_norm shape'


def test_every_exported_fifth_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax5_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_binding_checks_the_fifth_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT5_VERSION == 1

    class Old:   # a library from before the fifth table: the earlier ones are there and current
        def __getattr__(self, name):
            if name.startswith('cmdax5_'):
                raise AttributeError(name)
            return lambda *a: 1 if name in ('cmdax_abi_version', 'cmdax2_abi_version', 'cmdax3_abi_version', 'cmdax4_abi_version') else 0
    try:
        _lib._declare(Old())
    except _lib.CmdaError as e:
        assert 'cmdax5_' in str(e)
    else:
        raise AssertionError('a library without the fifth table must be rejected')

    class Stale(Old):   # the fifth table is there, at another version
        def __getattr__(self, name):
            if name == 'cmdax5_abi_version':
                return lambda *a: 2
            if name.startswith('cmdax5_'):
                return lambda *a: 0
            return Old.__getattr__(self, name)
    try:
        _lib._declare(Stale())
    except _lib.CmdaError as e:
        assert 'cmdax5_' in str(e) and 'version' in str(e)
    else:
        raise AssertionError('a fifth table of another version must be rejected')


_V = 'test_voxel_ordered.py'
KERNEL_TESTS = {
    'cmdax5_abi_version': ['test_abi_ext5.py::test_fifth_table_symbols_exported_by_hip_library'],
    'cmdax5_voxel_ordered_ws_bytes': ['test_abi_ext5.py::test_fifth_table_symbols_exported_by_hip_library',
                                      f'{_V}::test_voxel_ordered_ragged_batch'],
    'cmdax5_events_norm_ws_bytes': ['test_abi_ext5.py::test_fifth_table_symbols_exported_by_hip_library', f'{_V}::test_events_norm_batch'],
    'cmdax5_event_prep_batch': [f'{_V}::test_event_prep_batch_bitwise', f'{_V}::test_fifth_table_refusals'],
    'cmdax5_voxel_ordered': [f'{_V}::test_voxel_ordered_dense_cells_bitwise', f'{_V}::test_voxel_ordered_sparse_cells_bitwise',
                             f'{_V}::test_voxel_ordered_hot_pixel_bitwise', f'{_V}::test_voxel_ordered_segment_beyond_lds_bitwise',
                             f'{_V}::test_voxel_ordered_borders_bitwise', f'{_V}::test_voxel_ordered_ragged_batch',
                             f'{_V}::test_fifth_table_refusals'],
    'cmdax5_events_norm_batch': [f'{_V}::test_events_norm_batch', f'{_V}::test_fifth_table_refusals'],
}


def test_every_fifth_table_entry_point_has_a_kernel_level_test():
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
