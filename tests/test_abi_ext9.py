"""The ninth ABI extension (include/cmda_hip_ext9.h, prefix `cmdax9_`): the guarantees tests/test_abi_ext8.py gives the eighth one
(no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip_ext9.h')).read()
    return sorted(set(re.findall(r'\b(?:int|int64_t) (cmdax9_\w+)\(', text)))


def test_ninth_table_symbols_exported_by_hip_library():
    from cmda_amd._lib import Level9
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert syms == ['cmdax9_abi_version', 'cmdax9_feat_consis', 'cmdax9_ws_floats']
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip_ext9.h but not exported'
    assert lib.cmdax9_abi_version() == 1
    # the frozen tables do not move
    assert lib.cmdax8_abi_version() == 1 and lib.cmdax7_abi_version() == 1 and lib.cmdax6_abi_version() == 1
    assert lib.cmdax5_abi_version() == 1 and lib.cmdax4_abi_version() == 1 and lib.cmdax3_abi_version() == 1
    assert lib.cmdax2_abi_version() == 1 and lib.cmdax_abi_version() == 1 and lib.cmda_abi_version() == 8
    # the descriptor the binding fills is the header's: 3 pointers, 4 x int64, 2 x int32
    assert ctypes.sizeof(Level9) == 3 * 8 + 4 * 8 + 2 * 4
    i32, f32, vp = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
    lib.cmdax9_ws_floats.restype = ctypes.c_int64
    lib.cmdax9_ws_floats.argtypes = [vp, ctypes.c_int, ctypes.c_int]

    def levels(n=1, R=16, C=64, ld=None, fake=64, grad=True):
        arr = (Level9 * n)()
        for d in arr:
            d.a, d.b, d.grad, d.R, d.C = fake, fake, fake if grad else None, R, C
            d.lda = d.ldb = d.ldg = C if ld is None else ld
        return arr
    # the workspace query is decided on the host: one float per workgroup -- a workgroup per chunk of 512 threads x 4 sixteen-byte
    # pieces up to 256 chunks (129 here in bf16), then about 256 workgroups shared out by the levels' chunks (257 chunks in fp32)
    assert lib.cmdax9_ws_floats(levels(), 1, 0) == 1 and lib.cmdax9_ws_floats(levels(R=4099, C=512), 1, 0) == 256
    assert lib.cmdax9_ws_floats(levels(R=4099, C=512), 1, 1) == 129
    big = levels(2, R=2 ** 20, C=512)
    big[1].R = 1
    assert lib.cmdax9_ws_floats(big, 2, 0) == 256 + 1   # (every level keeps a workgroup of its own)
    four = levels(4)
    for d, (r, c) in zip(four, ((1024, 64), (256, 128), (64, 320), (15, 512))):
        d.R, d.C = r, c
    assert lib.cmdax9_ws_floats(four, 4, 1) == 4 + 2 + 2 + 1
    assert lib.cmdax9_ws_floats(levels(), 0, 0) == -1 and lib.cmdax9_ws_floats(levels(), 5, 0) == -1
    assert lib.cmdax9_ws_floats(levels(R=0), 1, 0) == -1 and lib.cmdax9_ws_floats(levels(C=0), 1, 0) == -1
    assert lib.cmdax9_ws_floats(None, 1, 0) == -1 and lib.cmdax9_ws_floats(levels(), 1, 2) == -1

    def call(arr, n=1, loss=vp(64), ticket=vp(64), ws=vp(64), fdt=0, gdt=0):
        return lib.cmdax9_feat_consis(arr, i32(n), f32(0.25), None, loss, vp(64), ticket, ws, i32(fdt), i32(gdt), None)
    # (the fake pointers are never dereferenced: every call below is refused on the host, before any HIP call)
    assert call(levels(), n=0) == -1 and call(levels(), n=5) == -1                      # n_levels outside 1..4
    assert call(levels(R=0)) == -1 and call(levels(C=0)) == -1 and call(levels(R=-3)) == -1   # R or C below 1
    assert call(levels(C=64, ld=63)) == -1                                              # a stride below C
    for name in ('lda', 'ldb', 'ldg'):
        arr = levels()
        setattr(arr[0], name, 8)
        assert call(arr) == -1, name
    arr = levels(grad=False)
    arr[0].ldg = 0                                                                      # (ldg is ignored without a gradient block)
    assert call(arr, loss=None) == -4                                                   # ... so the shape check passes and the pointers refuse
    assert call(levels(R=2 ** 31, C=4)) == -1                                           # pieces of a level at 2^31
    assert call(levels(), fdt=2) == -2 and call(levels(), gdt=3) == -2 and call(levels(), fdt=-1) == -2   # unknown dtype tag
    assert call(levels(), fdt=0, gdt=1) == -2                                           # bf16 gradient under fp32 features
    assert call(levels(C=0), fdt=2) == -1                                               # shapes first
    assert call(levels(grad=False), loss=None) == -4                                    # loss and every grad null at once
    assert call(None) == -4
    for name in ('a', 'b'):
        arr = levels()
        setattr(arr[0], name, None)
        assert call(arr) == -4, name
    assert call(levels(), ticket=None) == -4 and call(levels(), ws=None) == -4          # the loss needs its ticket and workspace


def test_every_exported_ninth_table_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" (?:int|int64_t) (cmdax9_\w+)\(', open(os.path.join(srcs, f)).read()))
    assert defined == set(declared_symbols())


def test_ninth_header_is_a_build_dependency():
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, re.M).group(1)
    assert 'include/cmda_hip_ext9.h' in hdrs.split()


def test_kernel_lives_with_the_hand_off_helper():
    """the last-workgroup hand-off has one definition, in feat_dist.hip, and the new kernel uses it there"""
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    text = open(os.path.join(srcs, 'feat_dist.hip')).read()
    assert len(re.findall(r'bool last_group\(', text)) == 1 and 'feat_consis_kernel' in text
    assert text.count('last_group(ticket') == 3   # the two feature-distance kernels and the feature-consistency kernel
    for f in os.listdir(srcs):
        if f != 'feat_dist.hip' and f.endswith(('.hip', '.h')):
            assert 'bool last_group(' not in open(os.path.join(srcs, f)).read(), f


def test_binding_checks_the_ninth_table_version():
    from cmda_amd import _lib
    assert _lib.ABI_EXT9_VERSION == 1

    class Old:   # a library from before the ninth table
        def __getattr__(self, name):
            if name.startswith('cmdax9_'):
                raise AttributeError(name)
            return lambda *a: 1
    try:
        _lib._declare_ext9(Old())
    except _lib.CmdaError as e:
        assert 'cmdax9_' in str(e) and 'lacks the ninth ABI table' in str(e)
    else:
        raise AssertionError('a library without the ninth table must be rejected')

    class Stale:   # the ninth table is there, at another version
        def __getattr__(self, name):
            if name == 'cmdax9_abi_version':
                return lambda *a: 2
            return type('Fn', (), {'__call__': lambda self, *a: 0})()
    try:
        _lib._declare_ext9(Stale())
    except _lib.CmdaError as e:
        assert 'cmdax9_' in str(e) and 'version' in str(e)
    else:
        raise AssertionError('a ninth table of another version must be rejected')

    class Current(Stale):
        def __getattr__(self, name):
            if name == 'cmdax9_abi_version':
                return lambda *a: 1
            return Stale.__getattr__(self, name)
    lib = Current()
    assert _lib._declare_ext9(lib) is lib
    # both loaders run the check on what the earlier checks return
    import inspect
    for fn in (_lib._load, _lib._bind_for_tests):
        assert '_declare_ext9(_declare_ext8(_declare(' in inspect.getsource(fn), fn.__name__


_T = 'test_feat_consis.py'
KERNEL_TESTS = {
    'cmdax9_abi_version': ['test_abi_ext9.py::test_ninth_table_symbols_exported_by_hip_library'],
    'cmdax9_ws_floats': ['test_abi_ext9.py::test_ninth_table_symbols_exported_by_hip_library', f'{_T}::test_feat_consis_against_float64'],
    'cmdax9_feat_consis': [f'{_T}::test_feat_consis_against_float64', f'{_T}::test_feat_consis_modes',
                           f'{_T}::test_feat_consis_strided_blocks', f'{_T}::test_feat_consis_refusals'],
}


def test_every_ninth_table_entry_point_has_a_kernel_level_test():
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
