"""ctypes binding of libcmda_hip.so (the C ABI declared in include/cmda_hip.h and its extensions include/cmda_hip_ext.h,
include/cmda_hip_ext2.h, include/cmda_hip_ext3.h, include/cmda_hip_ext4.h, include/cmda_hip_ext5.h, include/cmda_hip_ext6.h,
include/cmda_hip_ext7.h, include/cmda_hip_ext8.h and include/cmda_hip_ext9.h).

The product path has exactly one backend: the gfx950 kernel library built in-tree by
``__graft_entry__.build()`` / ``make hip``.  If it is missing, or a tensor is not on the GPU,
every op raises -- there is no CPU fallback.  ``_bind_for_tests`` exists only so that the
test-suite can run the *same kernel sources* through the CPU emulator build
(tests/emu/libcmda_emu.so); nothing in the package calls it.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CMDA_HIP_LIB: tuning builds of the SAME library (e.g. `make timing`); never a different backend
_LIB_PATH = os.environ.get('CMDA_HIP_LIB') or os.path.join(_HERE, 'libcmda_hip.so')

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

F32, BF16 = 0, 1
U8, I64 = 0, 1   # integer label tensors of the extension entry points (CMDAX_U8 / CMDAX_I64)
ABI_VERSION, ABI_EXT_VERSION = 8, 1
ABI_EXT2_VERSION = 1
ABI_EXT3_VERSION = 1
ABI_EXT4_VERSION = 1
ABI_EXT5_VERSION = 1
ABI_EXT6_VERSION = 1
ABI_EXT7_VERSION = 1
ABI_EXT8_VERSION = 1
ABI_EXT9_VERSION = 1


class View(ctypes.Structure):
    _fields_ = [('ptr', c_vp), ('ld', c_i64), ('R', c_i64), ('Cc', c_i64), ('batch_stride', c_i64), ('batch2_stride', c_i64),
                ('conv', c_i32), ('H', c_i32), ('W', c_i32), ('C', c_i32), ('OH', c_i32), ('OW', c_i32),
                ('KH', c_i32), ('KW', c_i32), ('stride', c_i32), ('pad', c_i32), ('dil', c_i32),
                ('in_dil', c_i32), ('reflect', c_i32), ('vec_ok', c_i32)]


class GemmParams(ctypes.Structure):
    _fields_ = [('A', View), ('B', View), ('a_kstrided', c_i32), ('b_kstrided', c_i32), ('C', c_vp),
                ('ldc', c_i64), ('c_batch_stride', c_i64), ('c_batch2_stride', c_i64), ('M', c_i32), ('N', c_i32),
                ('K', c_i32), ('batch', c_i32), ('batch2', c_i32), ('splits', c_i32), ('alpha', c_f32), ('beta', c_f32), ('bias', c_vp),
                ('act', c_i32), ('res', c_vp), ('ldres', c_i64), ('res_batch_stride', c_i64), ('res_batch2_stride', c_i64),
                ('rowscale', c_vp), ('rows_per_scale', c_i32), ('out_f32', c_i32), ('atomic', c_i32),
                ('dtype', c_i32), ('c_vec_ok', c_i32), ('colsum', c_vp),
                ('c_patch_ow', c_i32), ('c_patch_kh', c_i32), ('c_patch_kwci', c_i32), ('tile_hint', c_i32), ('c_perm_ci', c_i32), ('c_perm_cells', c_i32),
                ('res_f32', c_i32), ('colstats_rows', c_i32), ('colstats', c_vp)]


class Branch8(ctypes.Structure):   # cmdax8_branch_t
    _fields_ = [('z', c_vp), ('x', c_vp), ('mean', c_vp), ('rstd', c_vp), ('gamma', c_vp), ('beta', c_vp),
                ('dz', c_vp), ('dres', c_vp), ('dgamma', c_vp), ('dbeta', c_vp)]


class Level8(ctypes.Structure):    # cmdax8_level_t
    _fields_ = [('br', Branch8 * 2), ('out', c_vp), ('dout', c_vp), ('M', c_i64), ('C', c_i32), ('reserved', c_i32)]


class Level9(ctypes.Structure):    # cmdax9_level_t
    _fields_ = [('a', c_vp), ('b', c_vp), ('grad', c_vp), ('R', c_i64), ('lda', c_i64), ('ldb', c_i64), ('ldg', c_i64),
                ('C', c_i32), ('reserved', c_i32)]


class CmdaError(RuntimeError):
    pass


_ERR = {-1: 'bad shape', -2: 'unsupported dtype', -3: 'HIP launch error', -4: 'unsupported argument combination'}

_lib = None
_emulated = False


def _declare(lib):
    lib.cmda_abi_version.restype = ctypes.c_int
    lib.cmda_layernorm_bwd_ws_floats.restype = ctypes.c_int64
    lib.cmda_layernorm_bwd_ws_floats.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.cmda_bn_ws_floats.restype = ctypes.c_int64
    lib.cmda_bn_ws_floats.argtypes = [ctypes.c_int]
    lib.cmda_attention_bwd_ws_floats.restype = ctypes.c_int64
    lib.cmda_layernorm_slots.restype = ctypes.c_int
    lib.cmda_gemm_grouped_ws_bytes.restype = ctypes.c_int64
    # the extension table (include/cmda_hip_ext.h) is versioned on its own
    if not hasattr(lib, 'cmdax_abi_version'):
        raise CmdaError('the kernel library lacks the ABI extension (cmdax_*): rebuild it')
    lib.cmdax_abi_version.restype = ctypes.c_int
    if lib.cmdax_abi_version() != ABI_EXT_VERSION:
        raise CmdaError('libcmda_hip.so ABI extension version mismatch')
    # the second table (include/cmda_hip_ext2.h), again on its own
    if not hasattr(lib, 'cmdax2_abi_version'):
        raise CmdaError('the kernel library lacks the second ABI table (cmdax2_*): rebuild it')
    lib.cmdax2_abi_version.restype = ctypes.c_int
    if lib.cmdax2_abi_version() != ABI_EXT2_VERSION:
        raise CmdaError('libcmda_hip.so second ABI table (cmdax2_*) version mismatch')
    # the third table (include/cmda_hip_ext3.h): the ISR augmentations
    if not hasattr(lib, 'cmdax3_abi_version'):
        raise CmdaError('the kernel library lacks the third ABI table (cmdax3_*): rebuild it')
    lib.cmdax3_abi_version.restype = ctypes.c_int
    if lib.cmdax3_abi_version() != ABI_EXT3_VERSION:
        raise CmdaError('libcmda_hip.so third ABI table (cmdax3_*) version mismatch')
    lib.cmdax3_sky_mask_ws_bytes.restype = ctypes.c_int64
    lib.cmdax3_sky_mask_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    # the fourth table (include/cmda_hip_ext4.h): multi-parameter ISR and cow mask
    if not hasattr(lib, 'cmdax4_abi_version'):
        raise CmdaError('the kernel library lacks the fourth ABI table (cmdax4_*): rebuild it')
    lib.cmdax4_abi_version.restype = ctypes.c_int
    if lib.cmdax4_abi_version() != ABI_EXT4_VERSION:
        raise CmdaError('libcmda_hip.so fourth ABI table (cmdax4_*) version mismatch')
    lib.cmdax4_cow_mask_ws_bytes.restype = ctypes.c_int64
    lib.cmdax4_cow_mask_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    # the fifth table (include/cmda_hip_ext5.h): batched event prep, ordered voxel grid, batched events_norm
    if not hasattr(lib, 'cmdax5_abi_version'):
        raise CmdaError('the kernel library lacks the fifth ABI table (cmdax5_*): rebuild it')
    lib.cmdax5_abi_version.restype = ctypes.c_int
    if lib.cmdax5_abi_version() != ABI_EXT5_VERSION:
        raise CmdaError('libcmda_hip.so fifth ABI table (cmdax5_*) version mismatch')
    lib.cmdax5_voxel_ordered_ws_bytes.restype = ctypes.c_int64
    lib.cmdax5_voxel_ordered_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.cmdax5_events_norm_ws_bytes.restype = ctypes.c_int64
    lib.cmdax5_events_norm_ws_bytes.argtypes = [ctypes.c_int, ctypes.c_int64]
    # the sixth table (include/cmda_hip_ext6.h): the split train type's per-stream targets
    if not hasattr(lib, 'cmdax6_abi_version'):
        raise CmdaError('the kernel library lacks the sixth ABI table (cmdax6_*): rebuild it')
    lib.cmdax6_abi_version.restype = ctypes.c_int
    if lib.cmdax6_abi_version() != ABI_EXT6_VERSION:
        raise CmdaError('libcmda_hip.so sixth ABI table (cmdax6_*) version mismatch')
    # the seventh table (include/cmda_hip_ext7.h): the OHEM pixel sampler and its exact k-th-key select
    if not hasattr(lib, 'cmdax7_abi_version'):
        raise CmdaError('the kernel library lacks the seventh ABI table (cmdax7_*): rebuild it')
    lib.cmdax7_abi_version.restype = ctypes.c_int
    if lib.cmdax7_abi_version() != ABI_EXT7_VERSION:
        raise CmdaError('libcmda_hip.so seventh ABI table (cmdax7_*) version mismatch')
    lib.cmdax7_ws_bytes.restype = ctypes.c_int64
    lib.cmdax7_ws_bytes.argtypes = [ctypes.c_int64]
    return lib


def _declare_ext8(lib):
    """the eighth table (include/cmda_hip_ext8.h): the fused BasicBlock tail of ConvertAvgFusion.  Checked apart from `_declare`
    (whose contract ends with the seventh table); `_load` and `_bind_for_tests` call it right behind it."""
    if not hasattr(lib, 'cmdax8_abi_version'):
        raise CmdaError('the kernel library lacks the eighth ABI table (cmdax8_*): rebuild it')
    lib.cmdax8_abi_version.restype = ctypes.c_int
    if lib.cmdax8_abi_version() != ABI_EXT8_VERSION:
        raise CmdaError('libcmda_hip.so eighth ABI table (cmdax8_*) version mismatch')
    lib.cmdax8_ws_floats.restype = ctypes.c_int64
    lib.cmdax8_ws_floats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return lib


def _declare_ext9(lib):
    """the ninth table (include/cmda_hip_ext9.h): the feature-consistency loss.  Checked apart like the eighth; `_load` and
    `_bind_for_tests` call it around `_declare_ext8(_declare(...))`."""
    if not hasattr(lib, 'cmdax9_abi_version'):
        raise CmdaError('the kernel library lacks the ninth ABI table (cmdax9_*): rebuild it')
    lib.cmdax9_abi_version.restype = ctypes.c_int
    if lib.cmdax9_abi_version() != ABI_EXT9_VERSION:
        raise CmdaError('libcmda_hip.so ninth ABI table (cmdax9_*) version mismatch')
    lib.cmdax9_ws_floats.restype = ctypes.c_int64
    lib.cmdax9_ws_floats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return lib


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise CmdaError(
            f'{_LIB_PATH} not found: build the gfx950 kernel library first '
            '(python -c "import __graft_entry__ as g; g.build()" or `make hip`). '
            'cmda_amd has no CPU fallback.')
    _lib = _declare_ext9(_declare_ext8(_declare(ctypes.CDLL(_LIB_PATH))))
    if _lib.cmda_abi_version() != ABI_VERSION:
        raise CmdaError('libcmda_hip.so ABI version mismatch')
    return _lib


def _bind_for_tests(path):
    """TEST ONLY: route the C ABI to the CPU emulator build of the same kernel sources."""
    global _lib, _emulated
    _lib = _declare_ext9(_declare_ext8(_declare(ctypes.CDLL(path))))
    _emulated = True
    return _lib


def _unbind_for_tests():
    global _lib, _emulated
    _lib = None
    _emulated = False


def emulated():
    return _emulated


def lib():
    return _load()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_of(t):
    """the current HIP stream of t's device as a void* (raw handle: building a torch.cuda.Stream object per launch cost
    ~5 us of the ~14 us a launch spends in Python)"""
    if _emulated:
        return None
    if _raw_stream is not None:
        return c_vp(_raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device()))
    return c_vp(torch.cuda.current_stream(t.device).cuda_stream)


def check_dev(*tensors):
    for t in tensors:
        if t is None:
            continue
        if _emulated:
            if t.is_cuda:
                raise CmdaError('emulator build expects CPU tensors')
        elif not t.is_cuda:
            raise CmdaError('cmda_amd ops run only on the GPU (no CPU fallback); got a CPU tensor')
        if not t.is_contiguous():
            raise CmdaError('cmda_amd ops expect contiguous tensors')


def ptr(t):
    return c_vp(t.data_ptr()) if t is not None else None


def dtype_tag(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise CmdaError(f'unsupported activation dtype {t.dtype}')


def label_tag(t):
    if t.dtype == torch.uint8:
        return U8
    if t.dtype == torch.int64:
        return I64
    raise CmdaError(f'unsupported label dtype {t.dtype} (uint8 or int64)')


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise CmdaError(f'{name} failed: {_ERR.get(rc, rc)}')
