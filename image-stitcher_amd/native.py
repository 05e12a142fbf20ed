"""ctypes binding of libsquidstitch.so (include/squidstitch.h) -- the only way the host
reaches the device kernels.  PyTorch-ROCm tensors are used purely as device-buffer
containers: ``tensor.data_ptr()`` in, nothing torch-typed crosses the C-ABI.

There is no CPU fallback: if the shared object is missing or a call fails, this
module raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C image-stitcher_amd/csrc``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SQ_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libsquidstitch.so')

SQ_U8, SQ_U16, SQ_F32, SQ_F64 = 1, 2, 4, 8
SQ_ERR_INVALID, SQ_ERR_HIP, SQ_ERR_UNSUPPORTED, SQ_ERR_WORKSPACE, SQ_ERR_NUMERIC = -1, -2, -3, -4, -5
SQ_FUSE_OVERWRITE, SQ_FUSE_FEATHER = 0, 1
SQ_NORM_NONE, SQ_NORM_PHASE = 0, 1
SQ_FUSE_FORCE_QUEUES, SQ_FUSE_FORCE_STATIC, SQ_FUSE_NO_PLANE_GROUPS, SQ_FUSE_NO_SEAM_OWNERS, SQ_FUSE_CONSECUTIVE_GROUPS = 1, 2, 4, 8, 16
SQ_PROJECT_ACCUMULATE = 32
SQ_FOCUS_ACCUMULATE = 32
SQ_SELECT_ACCUMULATE = 32
SQ_FOCUS_MAX_RADIUS = 15
SQ_FOCUS_MAX_PLANES = 256
SQ_VERSION = 108
SQ_ARENA_NATURAL_ORDER = 1
SQ_ARENA_TWO_CLASSES = 2
SQ_ARENA_MAX_CLASSES = 8

RECT_DTYPE = np.dtype([('src_y0', '<i4'), ('src_x0', '<i4'), ('h', '<i4'), ('w', '<i4'),
                       ('dst_y', '<i4'), ('dst_x', '<i4')])
PAIR_DTYPE = np.dtype([('ref_tile', '<i4'), ('mov_tile', '<i4'), ('ref_y0', '<i4'), ('ref_x0', '<i4'),
                       ('mov_y0', '<i4'), ('mov_x0', '<i4')])
RESULT_DTYPE = np.dtype([('coarse', '<i4', (2,)), ('fine', '<i4', (2,)), ('ccmax_re', '<f8'),
                         ('ccmax_im', '<f8'), ('src_amp', '<f8'), ('tgt_amp', '<f8')])
SYNTH_DTYPE = np.dtype([('scene_seed', '<u8'), ('noise_seed', '<u8'), ('oy', '<i8'), ('ox', '<i8')])
OVERLAP_BATCH = 65535     # window pairs per sq_pair_overlap_moments call (include/squidstitch.h)
OVERLAP_DTYPE = np.dtype([('ref_tile', '<i4'), ('mov_tile', '<i4'), ('ref_y0', '<i4'), ('ref_x0', '<i4'),
                          ('mov_y0', '<i4'), ('mov_x0', '<i4'), ('h', '<i4'), ('w', '<i4')])


class NativeError(RuntimeError):
    """A libsquidstitch call returned a negative status (``status``: the sq_status code, when the call gave one)."""

    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


class _FuseArgs(C.Structure):
    _fields_ = [
        ('plan', C.c_void_p), ('table_dev', C.c_void_p), ('table_bytes', C.c_int64),
        ('tile_ptrs_dev', C.c_void_p), ('tile_base_dev', C.c_void_p),
        ('tile_plane_stride', C.c_int64), ('tile_stride', C.c_int64),
        ('n_tiles', C.c_int32), ('tile_h', C.c_int32), ('tile_w', C.c_int32),
        ('tile_pitch', C.c_int32), ('tile_dtype', C.c_int32),
        ('flat_ptrs_dev', C.c_void_p), ('flat_dtype', C.c_int32),
        ('canvas_dev', C.c_void_p), ('canvas_plane_stride', C.c_int64),
        ('canvas_h', C.c_int32), ('canvas_w', C.c_int32), ('canvas_pitch', C.c_int32),
        ('canvas_dtype', C.c_int32), ('n_planes', C.c_int32), ('mode', C.c_int32),
        ('scratch_dev', C.c_void_p), ('scratch_bytes', C.c_int64),
        ('flags', C.c_int32), ('grid_blocks', C.c_int32),
    ]


class _FocusArgs(C.Structure):
    _fields_ = [
        ('z_levels_dev', C.c_void_p), ('radius', C.c_int32),
        ('scratch_dev', C.c_void_p), ('scratch_bytes', C.c_int64),
        ('key_dev', C.c_void_p), ('key_pitch', C.c_int32),
    ]


class _RegisterArgs(C.Structure):
    _fields_ = [
        ('tile_ptrs_dev', C.c_void_p), ('tile_base_dev', C.c_void_p), ('tile_stride', C.c_int64),
        ('n_tiles', C.c_int32), ('tile_h', C.c_int32), ('tile_w', C.c_int32),
        ('tile_pitch', C.c_int32), ('tile_dtype', C.c_int32),
        ('minmax_dev', C.c_void_p), ('pairs_dev', C.c_void_p), ('n_pairs', C.c_int32),
        ('n0', C.c_int32), ('n1', C.c_int32), ('upsample_factor', C.c_int32), ('normalization', C.c_int32),
        ('results_dev', C.c_void_p), ('workspace_dev', C.c_void_p), ('workspace_bytes', C.c_int64),
    ]


class _RegisterPlan(C.Structure):
    _fields_ = [
        ('m0', C.c_int32), ('m1', C.c_int32), ('long0', C.c_int32), ('long1', C.c_int32),
        ('gen0', C.c_int32), ('gen1', C.c_int32), ('nf0', C.c_int32), ('nf1', C.c_int32),
        ('radix0', C.c_uint8 * 16), ('radix1', C.c_uint8 * 16),
        ('tc', C.c_int32), ('share', C.c_int32), ('col_threads', C.c_int32),
        ('columns_single', C.c_int32), ('columns_single_threads', C.c_int32),
        ('rl_fwd', C.c_int32), ('rl_inv', C.c_int32), ('threads_fwd', C.c_int32), ('threads_inv', C.c_int32),
        ('upsample_rows_tb', C.c_int32), ('upsample_rows_kc', C.c_int32),
        ('grid_fwd', C.c_int32 * 2), ('grid_col', C.c_int32 * 2), ('grid_inv', C.c_int32 * 2),
        ('grid_up_rows', C.c_int32 * 2),
        ('lds_fwd', C.c_int64), ('lds_col', C.c_int64), ('lds_inv', C.c_int64),
    ]


class _ArenaInfo(C.Structure):
    _fields_ = [('base_dev', C.c_void_p), ('bytes', C.c_int64), ('slice_bytes', C.c_int64), ('n_slices', C.c_int32),
                ('n_candidates', C.c_int32), ('n_classes', C.c_int32), ('class_slices', C.c_int32 * 8),
                ('class_candidates', C.c_int32 * 8), ('interleaved', C.c_int32),
                ('probe_ms', C.c_float), ('create_ms', C.c_float), ('min_pair_gbs', C.c_float), ('max_pair_gbs', C.c_float)]


class _BasicInfo(C.Structure):
    _fields_ = [('reweight_iterations', C.c_int32), ('ladmap_iterations', C.c_int32), ('working_size', C.c_int32),
                ('capped_rounds', C.c_int32)]


EXPORTS = {
    'sq_version': (C.c_int, []),
    'sq_last_error': (C.c_char_p, []),
    'sq_fuse_plan_create': (C.c_void_p, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'sq_fuse_plan_create_spans': (C.c_void_p, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'sq_fuse_plan_expand_scratch_bytes': (C.c_int64, [C.c_void_p]),
    'sq_fuse_plan_expand': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    'sq_fuse_plan_destroy': (None, [C.c_void_p]),
    'sq_fuse_plan_table_bytes': (C.c_int64, [C.c_void_p]),
    'sq_fuse_plan_upload': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'sq_fuse_plan_export': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'sq_fuse_plan_stats': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'sq_fuse_planes': (C.c_int, [C.POINTER(_FuseArgs), C.c_void_p]),
    'sq_fuse_project_max': (C.c_int, [C.POINTER(_FuseArgs), C.c_int32, C.c_void_p]),
    'sq_focus_scratch_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    'sq_fuse_project_focus': (C.c_int, [C.POINTER(_FuseArgs), C.POINTER(_FocusArgs), C.c_int32, C.c_void_p]),
    'sq_focus_depth_plane': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'sq_fuse_select_depth': (C.c_int, [C.POINTER(_FuseArgs), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'sq_tile_minmax': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_pair_overlap_moments': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_normalize_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sq_downsample2': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                 C.c_int32, C.c_int32, C.c_void_p]),
    'sq_pyramid_mean': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'sq_histogram_planes': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                      C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_block_mean': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'sq_composite_render': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_void_p, C.c_int64, C.c_void_p]),
    'sq_tophat_scratch_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'sq_tophat_tiles': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_int64, C.c_void_p]),
    'sq_despeckle_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_tile_stats': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_seam_stats': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_dpc_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                               C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    'sq_bin_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                               C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'sq_warp_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                C.c_int32, C.c_int32, C.c_void_p]),
    'sq_shift_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                 C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    'sq_affine_tiles': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    'sq_dark_tiles': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p]),
    'sq_register_line_supported': (C.c_int, [C.c_int32]),
    'sq_register_workspace_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'sq_register_pairs': (C.c_int, [C.POINTER(_RegisterArgs), C.c_void_p]),
    'sq_register_describe': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_RegisterPlan)]),
    'sq_selftest_flat_divide': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_selftest_flat_divide_f64': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]),
    'sq_selftest_normalise_divide': (C.c_int, [C.c_void_p, C.c_void_p]),
    'sq_selftest_blend_divide': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'sq_fuse_scratch_bytes': (C.c_int64, [C.c_int32]),
    'sq_arena_create': (C.c_void_p, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(_ArenaInfo)]),
    'sq_arena_info_get': (C.c_int, [C.c_void_p, C.POINTER(_ArenaInfo)]),
    'sq_arena_destroy': (C.c_int, [C.c_void_p]),
    'sq_write_files': (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    'sq_blosc_chunk_count': (C.c_int64, [C.c_int32] * 5),
    'sq_blosc_out_bound': (C.c_int64, [C.c_int32] * 6),
    'sq_blosc_scratch_bytes': (C.c_int64, [C.c_int32] * 6),
    'sq_blosc_encode_planes': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'sq_deflate_chunk_count': (C.c_int64, [C.c_int32] * 5),
    'sq_deflate_out_bound': (C.c_int64, [C.c_int32] * 6),
    'sq_deflate_scratch_bytes': (C.c_int64, [C.c_int32] * 6),
    'sq_deflate_encode_planes': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p]),
    'sq_jpeg_chunk_count': (C.c_int64, [C.c_int32] * 5),
    'sq_jpeg_out_bound': (C.c_int64, [C.c_int32] * 6),
    'sq_jpeg_scratch_bytes': (C.c_int64, [C.c_int32] * 6),
    'sq_jpeg_encode_planes': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p]),
    'sq_basic_workspace_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    'sq_basic_fit': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_BasicInfo), C.c_void_p]),
    'sq_synth_tiles': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libsquidstitch.so once; fail loudly when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # PyTorch-ROCm ships its own libamdhip64.so.7; loading it first makes this library bind to
        # the SAME HIP runtime (same SONAME) instead of bringing /opt/rocm's copy in beside it --
        # two runtimes in one process cannot see each other's device allocations.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(handle, name)   # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if handle.sq_version() != SQ_VERSION:
            raise NativeError(f"{LIB_PATH} is version {handle.sq_version()}, this binding expects {SQ_VERSION}: rebuild it")
        _lib = handle
    return _lib


def _check(status: int, what: str) -> None:
    if status < 0:
        raise NativeError(f"{what} failed ({status}): {lib().sq_last_error().decode()}", status)


def _size(n, what: str) -> int:
    """The result of a size query (sq_*_bytes and their like): a negative one is the status of a query that failed."""
    n = int(n)
    _check(n, what)
    return n


def _int_in(value, lo: int, hi: int, what: str) -> int:
    """``value`` as an int when it is a Python or numpy integer (no bool, no float) in lo..hi; ValueError otherwise."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{what} must be an integer in {lo}..{hi}, got {value!r}")
    return int(value)


def sq_dtype_of(np_dtype) -> int:
    dt = np.dtype(np_dtype)
    table = {np.dtype('uint8'): SQ_U8, np.dtype('uint16'): SQ_U16, np.dtype('float32'): SQ_F32,
             np.dtype('float64'): SQ_F64}
    if dt not in table:
        raise ValueError(f"unsupported dtype {dt} (uint8/uint16 tiles, float32/float64 gains)")
    return table[dt]


def torch_dtype_of(np_dtype):
    import torch
    return {np.dtype('uint8'): torch.uint8, np.dtype('uint16'): torch.uint16,
            np.dtype('float32'): torch.float32, np.dtype('float64'): torch.float64}[np.dtype(np_dtype)]


def np_dtype_of_torch(t) -> np.dtype:
    import torch
    return {torch.uint8: np.dtype('uint8'), torch.uint16: np.dtype('uint16'),
            torch.float32: np.dtype('float32'), torch.float64: np.dtype('float64')}[t]


def _stream_ptr(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _on_stream(stream):
    """Makes ``stream`` the current stream for a wrapper's allocations, zero-fills, uploads and launch: outputs, scratch,
    workspaces and result buffers are then made, cleared and used on the stream the kernels run on (a buffer taken from
    another stream's pool could be handed out again while they still run, and a zero-fill on another stream lands whenever
    that stream gets to it).  None: the current stream is the one the kernels run on already."""
    if stream is None:
        return contextlib.nullcontext()
    import torch
    return torch.cuda.stream(stream)


def as_rects(rects) -> np.ndarray:
    """[n, 6] ints (src_y0, src_x0, h, w, dst_y, dst_x) or a RECT_DTYPE array -> RECT_DTYPE."""
    if isinstance(rects, np.ndarray) and rects.dtype == RECT_DTYPE:
        return np.ascontiguousarray(rects)
    a = np.asarray(rects, dtype=np.int64).reshape(-1, 6)
    if a.size and (np.abs(a) >= 2 ** 31).any():
        raise ValueError("rectangle coordinate does not fit int32")
    out = np.zeros(len(a), dtype=RECT_DTYPE)
    for i, name in enumerate(RECT_DTYPE.names):
        out[name] = a[:, i]
    return out


# Largest tile height whose overwrite plan the device can expand (csrc/plan_expand.hip: MAX_BUCKETS row blocks of 8 rows)
EXPAND_MAX_TILE_H = 8176


class FusePlan:
    """Host handle of one fusion plan (sq_fuse_plan_*).  ``table`` is the byte image the
    device reads; ``device_table(device)`` uploads it once and caches the tensor.

    ``expand_on_device=True`` (overwrite plans): the host stops after the sweep into spans and ``device_table`` has the
    work list -- items, seam owners, their order -- produced by kernels in device memory (sq_fuse_plan_create_spans /
    sq_fuse_plan_expand; the table is the host planner's byte for byte, tests/test_plan_gpu.py): what a job pays between
    registration and its first fusion launch drops from ~5.5 ms + a 14.7 MB upload to ~1.5 ms for a 32 x 32 grid.
    ``device_table`` is serialised per plan (the expansion writes the plan's host header), and a table whose expansion or
    upload failed is not kept: the next call starts over."""

    def __init__(self, rects, tile_h: int, tile_w: int, canvas_h: int, canvas_w: int, mode: int = SQ_FUSE_OVERWRITE,
                 expand_on_device: bool = False):
        L = lib()
        self.rects = as_rects(rects)
        self.tile_h, self.tile_w = int(tile_h), int(tile_w)
        self.canvas_h, self.canvas_w = int(canvas_h), int(canvas_w)
        self.mode = int(mode)
        self.n_tiles = len(self.rects)
        self.expand_on_device = bool(expand_on_device) and self.mode == SQ_FUSE_OVERWRITE and self.tile_h <= EXPAND_MAX_TILE_H
        create = L.sq_fuse_plan_create_spans if self.expand_on_device else L.sq_fuse_plan_create
        self._h = create(self.rects.ctypes.data if self.n_tiles else None, self.n_tiles,
                         self.tile_h, self.tile_w, self.canvas_h, self.canvas_w, self.mode)
        if not self._h:
            raise NativeError(f"sq_fuse_plan_create failed: {L.sq_last_error().decode()}")
        self.table_bytes = int(L.sq_fuse_plan_table_bytes(self._h))
        self._table = None
        ns, ni, cv, mr = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _check(L.sq_fuse_plan_stats(self._h, C.byref(ns), C.byref(ni), C.byref(cv), C.byref(mr)), 'sq_fuse_plan_stats')
        self.n_spans, self.n_items, self.covered_voxels, self.max_refs = ns.value, ni.value, cv.value, mr.value
        self._dev = {}
        import threading
        self._lock = threading.Lock()

    @property
    def handle(self) -> int:
        return self._h

    @property
    def table(self) -> np.ndarray:
        """Host copy of the byte image the device reads (tests, inspection)."""
        if self._table is None:
            if self.expand_on_device:      # the items exist on the device only: read the expanded table back
                if not self._dev:
                    raise NativeError("FusePlan.table: a plan expanded on the device has no host copy before device_table() has run")
                self._table = next(iter(self._dev.values())).cpu().numpy()
            else:
                self._table = np.empty(self.table_bytes, dtype=np.uint8)
                _check(lib().sq_fuse_plan_export(self._h, self._table.ctypes.data, self.table_bytes), 'sq_fuse_plan_export')
        return self._table

    def device_table(self, device):
        """The table in device memory, uploaded once per device (one DMA from the plan's page-locked
        storage; sq_fuse_plan_upload waits for it, so the plan can be dropped at any time)."""
        import torch
        key = str(device)
        with self._lock:      # sq_fuse_plan_expand writes the plan's host header: one expansion (or upload) at a time per plan
            return self._device_table_locked(key, device)

    def _device_table_locked(self, key, device):
        import torch
        if key not in self._dev:
            # on the read-back / upload stream, not the caller's: the copy must not queue behind a fusion
            # launch that is still running there (the entry point waits for the copy, so the table is
            # complete before anything later is launched).  The block comes from THAT stream's pool (see
            # _side_empty): a block of the caller's pool could still be read by a running fusion kernel.
            dev = _side_empty((max(self.table_bytes, 1),), torch.uint8, torch.device(device))
            with torch.cuda.device(dev.device):
                side = _copy_stream(dev.device)
                if self.expand_on_device:
                    need = _size(lib().sq_fuse_plan_expand_scratch_bytes(self._h), 'sq_fuse_plan_expand_scratch_bytes')
                    with torch.cuda.stream(side):      # written and read on the side stream only, dropped on return
                        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev.device)
                    _check(lib().sq_fuse_plan_expand(self._h, dev.data_ptr(), dev.numel(), scratch.data_ptr(), scratch.numel(),
                                                     _stream_ptr(side)), 'sq_fuse_plan_expand')
                    del scratch
                else:
                    _check(lib().sq_fuse_plan_upload(self._h, dev.data_ptr(), dev.numel(), _stream_ptr(side)), 'sq_fuse_plan_upload')
            self._dev[key] = dev
        else:
            self._dev[key].record_stream(torch.cuda.current_stream(self._dev[key].device))
        return self._dev[key]

    def close(self) -> None:
        if getattr(self, '_h', None):
            lib().sq_fuse_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _side_empty(shape, dtype, device):
    """Device tensor that is WRITTEN on the copy stream and READ by kernels on the caller's stream.

    The block is taken from the copy stream's pool and ``record_stream``-ed for the caller's stream, so the
    caching allocator hands it out again only after the caller-stream work enqueued up to the moment it is
    dropped has finished -- and then only to another copy-stream allocation.  (Allocated from the caller's
    pool instead, a dropped block would be reused by the next upload at once and overwritten from the copy
    stream while a fusion kernel launched earlier is still reading it.)"""
    import torch
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.stream(_copy_stream(device)):
        t = torch.empty(shape, dtype=dtype, device=device)
    t.record_stream(torch.cuda.current_stream(device))
    return t


def upload_small(host, device):
    """A small host tensor -> device, copied on the read-back / upload stream instead of the caller's: a
    pageable host-to-device copy blocks the host until everything queued before it on ITS stream is done,
    and on the caller's stream that can be a 35 ms fusion launch.  Returns when the data is on the device."""
    import torch
    dst = _side_empty(tuple(host.shape), host.dtype, device)
    if dst.numel():
        with torch.cuda.stream(_copy_stream(dst.device)):
            dst.copy_(host)      # pageable source: returns when the bytes are on the device
    return dst


def pointer_table(tensors: Sequence, device):
    """Device int64 tensor of data_ptr()s (0 for None); the caller keeps ``tensors`` alive."""
    import torch
    ptrs = [0 if t is None else int(t.data_ptr()) for t in tensors]
    return upload_small(torch.tensor(ptrs, dtype=torch.int64), device)


def _fuse_args(plan: FusePlan, tiles, n_planes: int, out, plane_stride: int, pitch: int, flats, tile_ptrs, flat_ptrs, keep):
    """The sq_fuse_args of ``n_planes`` planes of ``tiles`` (or ``tile_ptrs``) into ``out`` (its geometry given by the caller)."""
    import torch
    L = lib()
    hc, wc = int(out.shape[-2]), int(out.shape[-1])
    a = _FuseArgs()
    a.plan = plan.handle
    table = plan.device_table(out.device)
    a.table_dev = table.data_ptr()
    a.table_bytes = table.numel()
    keep.append(table)
    if tile_ptrs is not None:
        if tile_ptrs.dtype != torch.int64 or tile_ptrs.numel() != n_planes * plan.n_tiles:
            raise ValueError("tile_ptrs must be int64 with n_planes * n_tiles entries")
        a.tile_ptrs_dev = tile_ptrs.data_ptr()
        a.tile_base_dev = None
        tile_np = np_dtype_of_torch(out.dtype) if plan.mode == SQ_FUSE_OVERWRITE else np.dtype('uint16')
        if tiles is not None:
            tile_np = np_dtype_of_torch(tiles.dtype)
    else:
        if tiles is None or not tiles.is_cuda or not tiles.is_contiguous():
            raise ValueError("tiles must be a contiguous device tensor")
        if tiles.numel() != n_planes * plan.n_tiles * plan.tile_h * plan.tile_w:
            raise ValueError(f"tiles has {tiles.numel()} elements, expected "
                             f"{n_planes}x{plan.n_tiles}x{plan.tile_h}x{plan.tile_w}")
        a.tile_ptrs_dev = None
        a.tile_base_dev = tiles.data_ptr()
        a.tile_stride = plan.tile_h * plan.tile_w
        a.tile_plane_stride = plan.n_tiles * plan.tile_h * plan.tile_w
        tile_np = np_dtype_of_torch(tiles.dtype)
    a.n_tiles, a.tile_h, a.tile_w, a.tile_pitch = plan.n_tiles, plan.tile_h, plan.tile_w, plan.tile_w
    a.tile_dtype = sq_dtype_of(tile_np)
    a.flat_ptrs_dev = None
    a.flat_dtype = SQ_F32
    if flats is not None and any(f is not None for f in flats):
        if len(flats) != n_planes:
            raise ValueError("flats needs one entry per plane")
        dts = {f.dtype for f in flats if f is not None}
        if len(dts) != 1:
            raise ValueError("all flatfields must share one dtype")
        for f in flats:
            if f is not None and (tuple(f.shape) != (plan.tile_h, plan.tile_w) or not f.is_contiguous()):
                raise ValueError("flatfield must be a contiguous tile_h x tile_w tensor")
        a.flat_dtype = sq_dtype_of(np_dtype_of_torch(dts.pop()))
        fp = flat_ptrs if flat_ptrs is not None else pointer_table(flats, out.device)
        if fp.dtype != torch.int64 or fp.numel() != n_planes:
            raise ValueError("flat_ptrs must be int64 with one entry per plane")
        keep.append(fp)
        a.flat_ptrs_dev = fp.data_ptr()
    if n_planes > 0:   # gain classes + work-queue counters (torch allocations are 512-byte aligned)
        scratch = torch.empty(int(L.sq_fuse_scratch_bytes(n_planes)), dtype=torch.uint8, device=out.device)
        keep.append(scratch)
        a.scratch_dev = scratch.data_ptr()
        a.scratch_bytes = scratch.numel()
    a.canvas_dev = out.data_ptr()
    a.canvas_plane_stride = plane_stride
    a.canvas_h, a.canvas_w, a.canvas_pitch = hc, wc, pitch
    a.canvas_dtype = sq_dtype_of(np_dtype_of_torch(out.dtype))
    a.n_planes = n_planes
    a.mode = plan.mode
    return a


def _fuse_launch(name: str, stream, keep, plan: FusePlan, tiles, n_planes: int, out, plane_stride: int, pitch: int, flats, tile_ptrs,
                 flat_ptrs, *rest, flags: int = 0, grid_blocks: int = 0) -> None:
    """The launch every fuse wrapper ends with, called inside its ``_on_stream(stream)``: the sq_fuse_args (``_fuse_args``) with
    ``flags`` and ``grid_blocks``, everything in ``keep`` (the wrapper's own buffers and the ones made here) recorded on
    ``stream``, then entry point ``name``(args, *rest, stream)."""
    a = _fuse_args(plan, tiles, n_planes, out, plane_stride, pitch, flats, tile_ptrs, flat_ptrs, keep)
    a.flags, a.grid_blocks = int(flags), int(grid_blocks)
    if stream is not None:      # launched on another stream than the one the helpers above allocated for
        for t in keep:
            t.record_stream(stream)
    _check(getattr(lib(), name)(C.byref(a), *rest, _stream_ptr(stream)), name)


def _check_plane(name, t, shape) -> int:
    """The row pitch of ``t``, a [Hc, Wc] device tensor of this shape with unit-stride rows; ValueError otherwise."""
    if not t.is_cuda or t.dim() != 2 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a [{shape[0]}, {shape[1]}] device tensor")
    if (shape[1] > 1 and t.stride(1) != 1) or (shape[0] > 1 and t.stride(0) < shape[1]):
        raise ValueError(f"{name} must have unit-stride rows")
    return int(t.stride(0)) if shape[0] > 1 else int(shape[1])


def _projected_planes(plan, tiles, tile_ptrs, flats) -> int:
    """The number of z planes a projection call was given: tiles.shape[0], or what the pointer table holds per tile."""
    if tile_ptrs is not None:
        return int(tile_ptrs.numel()) // plan.n_tiles if plan.n_tiles else (len(flats) if flats is not None else 1)
    if tiles is not None:
        return int(tiles.shape[0]) if tiles.dim() == 4 else 1
    raise ValueError("tiles or tile_ptrs is required")


def _z_level_words(z_levels, distinct: bool) -> np.ndarray:
    """Host z levels (a sequence or a host tensor), each in 0 .. 2^32 - 1, as the int32 words the device reads as uint32."""
    zs = [int(z) for z in (z_levels.tolist() if hasattr(z_levels, 'tolist') else z_levels)]
    if any(not 0 <= z < 2 ** 32 for z in zs):
        raise ValueError("z levels must lie in 0 .. 2^32 - 1")
    if distinct and len(set(zs)) != len(zs):
        raise ValueError("the z levels of a call must be distinct")
    return np.array(zs, dtype=np.uint32).view(np.int32)


def _z_levels_dev(z_levels, n_planes: int, device, distinct: bool = False):
    """Device int32 tensor of the z levels of a call's ``n_planes`` planes (a device tensor is converted, not checked)."""
    import torch
    if torch.is_tensor(z_levels) and z_levels.is_cuda:
        zl = z_levels.to(torch.int32)
    else:
        zl = upload_small(torch.tensor(_z_level_words(z_levels, distinct)), device)
    if zl.numel() != n_planes:
        raise ValueError(f"{zl.numel()} z levels for {n_planes} planes")
    return zl


def fuse_planes(plan: FusePlan, tiles, canvas, flats=None, tile_ptrs=None, stream=None, flat_ptrs=None,
                flags: int = 0, grid_blocks: int = 0) -> None:
    """Fuse all planes of ``canvas`` ([P, Hc, Wc] or [..., Hc, Wc] contiguous) from ``tiles``.

    tiles:     contiguous device tensor [P, N, H, W] (N = plan.n_tiles), or None with
               ``tile_ptrs`` = device int64 tensor [P*N] of tile pointers (dense H x W tiles).
    flats:     None, or a list of P device tensors / None (H x W float32 or float64 gains);
               all non-None entries must share one dtype.
    flat_ptrs: optionally ``pointer_table(flats, device)`` made earlier, for callers that fuse with the same
               gains again and again (saves a small blocking upload per call).
    """
    hc, wc = int(canvas.shape[-2]), int(canvas.shape[-1])
    n_planes = int(canvas.numel() // (hc * wc)) if hc * wc else 0
    # contiguous, or [P, Hc, Wc] with dense rows and any row pitch / plane stride (empty_canvas pads the plane stride)
    pitch, plane_stride = wc, hc * wc
    if not canvas.is_cuda:
        raise ValueError("canvas must be a device tensor")
    if not canvas.is_contiguous():
        if canvas.dim() != 3 or (wc > 1 and canvas.stride(2) != 1) or canvas.stride(1) < wc or \
                (n_planes > 1 and canvas.stride(0) < (hc - 1) * canvas.stride(1) + wc):
            raise ValueError("canvas must be contiguous or a [P, Hc, Wc] tensor with unit-stride rows and non-overlapping planes")
        pitch, plane_stride = int(canvas.stride(1)), int(canvas.stride(0))
    with _on_stream(stream):
        _fuse_launch('sq_fuse_planes', stream, [], plan, tiles, n_planes, canvas, plane_stride, pitch, flats, tile_ptrs, flat_ptrs,
                     flags=flags, grid_blocks=grid_blocks)


def fuse_project_max(plan: FusePlan, tiles, out, flats=None, tile_ptrs=None, accumulate: bool = False, flags: int = 0,
                     stream=None, flat_ptrs=None, grid_blocks: int = 0) -> None:
    """Maximum-intensity projection over z (sq_fuse_project_max; an extension, the reference has none): ``out`` ([Hc, Wc]
    device tensor with unit-stride rows, the tile dtype) = the per-voxel maximum over the Z planes of ``tiles`` of what
    ``fuse_planes`` would store in each plane -- bit for bit ``fuse_planes(...)`` followed by ``amax`` over z, without the stack.

    tiles / tile_ptrs / flats / flat_ptrs: as in ``fuse_planes`` with P = Z planes (Z = tiles.shape[0], or
    tile_ptrs.numel() // plan.n_tiles).  The plan must be an overwrite plan.
    accumulate: ``out`` = max(out, projection) on the plan's covered voxels, the uncovered ones untouched (a channel's z planes
    that come in several calls or under different plans); otherwise every voxel of ``out`` is written, uncovered ones 0."""
    if plan.mode != SQ_FUSE_OVERWRITE:
        raise ValueError("fuse_project_max projects overwrite plans only")
    pitch = _check_plane('out', out, (plan.canvas_h, plan.canvas_w))
    n_planes = _projected_planes(plan, tiles, tile_ptrs, flats)
    if n_planes < 1:
        raise ValueError("at least one plane to project")
    with _on_stream(stream):
        _fuse_launch('sq_fuse_project_max', stream, [], plan, tiles, n_planes, out, 0, pitch, flats, tile_ptrs, flat_ptrs,
                     int(flags) | (SQ_PROJECT_ACCUMULATE if accumulate else 0), grid_blocks=grid_blocks)


def focus_scratch_bytes(n_tiles: int, tile_h: int, tile_w: int) -> int:
    """Bytes of the caller-owned scratch of ``fuse_project_focus`` for a plan of ``n_tiles`` tiles of tile_h x tile_w: the
    per-tile-pixel winner (uint32 score + uint8 plane index), about 5 B per tile pixel whatever the number of planes."""
    return _size(lib().sq_focus_scratch_bytes(int(n_tiles), int(tile_h), int(tile_w)), 'sq_focus_scratch_bytes')


def fuse_project_focus(plan: FusePlan, tiles, out, key, z_levels, radius: int = 3, flats=None, scratch=None,
                       accumulate: bool = False, tile_ptrs=None, flags: int = 0, stream=None, flat_ptrs=None,
                       grid_blocks: int = 0) -> None:
    """Best-focus (extended depth of field) projection over z (sq_fuse_project_focus; an extension, the reference has none).
    Per tile pixel the focus score F = the (2R+1)^2 box sum of the modified Laplacian of the RAW tile (reads clamped to the
    full staged tile); per canvas voxel the plane with the largest key (F << 32) | (0xFFFFFFFF - z) among the planes whose
    owner pixel covers it -- the highest score, on a tie the lowest z level -- and ``out`` = what ``fuse_planes`` stores for
    that plane there (the same flatfield divide), ``key`` = that key.  Uncovered voxels: 0 in both.

    out:      [Hc, Wc] device tensor of the tile dtype with unit-stride rows.
    key:      [Hc, Wc] device int64 tensor with unit-stride rows (the keys are < 2^63); depth = 0xFFFFFFFF - (key & 0xFFFFFFFF).
    z_levels: the z level of each of the call's Z planes (a sequence, or a device int64 / int32 tensor); 0 <= z < 2^32.
    radius:   R, 0..15.
    tiles / tile_ptrs / flats / flat_ptrs: as in ``fuse_project_max`` (Z = tiles.shape[0]; at most 256 planes per call).
    scratch:  optional device uint8 tensor of at least ``focus_scratch_bytes(plan.n_tiles, tile_h, tile_w)`` bytes (reuse it
              across calls); allocated here when None.
    accumulate: voxels whose new key exceeds ``key`` take the new value and key, the others (and uncovered voxels) stay --
              the z planes of a channel that come in several calls, in any z order, or under different plans."""
    import torch
    if plan.mode != SQ_FUSE_OVERWRITE:
        raise ValueError("fuse_project_focus projects overwrite plans only")
    if not 0 <= int(radius) <= SQ_FOCUS_MAX_RADIUS:
        raise ValueError(f"focus radius {radius} outside 0..{SQ_FOCUS_MAX_RADIUS}")
    shape = (plan.canvas_h, plan.canvas_w)
    pitch = _check_plane('out', out, shape)
    key_pitch = _check_plane('key', key, shape)
    if key.dtype != torch.int64:
        raise ValueError("key must be an int64 tensor")
    n_planes = _projected_planes(plan, tiles, tile_ptrs, flats)
    if not 1 <= n_planes <= SQ_FOCUS_MAX_PLANES:
        raise ValueError(f"{n_planes} planes: a call projects 1..{SQ_FOCUS_MAX_PLANES}")
    with _on_stream(stream):
        zl = _z_levels_dev(z_levels, n_planes, out.device)
        need = focus_scratch_bytes(plan.n_tiles, plan.tile_h, plan.tile_w)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.uint8, device=out.device)
        elif scratch.numel() * scratch.element_size() < need or not scratch.is_cuda:
            raise ValueError(f"focus scratch must be a device tensor of at least {need} bytes")
        f = _FocusArgs()
        f.z_levels_dev = zl.data_ptr()
        f.radius = int(radius)
        f.scratch_dev, f.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
        f.key_dev, f.key_pitch = key.data_ptr(), key_pitch
        _fuse_launch('sq_fuse_project_focus', stream, [zl, scratch], plan, tiles, n_planes, out, 0, pitch, flats, tile_ptrs,
                     flat_ptrs, C.byref(f), int(flags) | (SQ_FOCUS_ACCUMULATE if accumulate else 0), grid_blocks=grid_blocks)


def depth_of_keys(key):
    """The winning z level of each voxel of a key plane (``fuse_project_focus``): 0xFFFFFFFF - the low word, -1 where the key
    is 0 (no plane covers the voxel).  int64, torch or numpy like ``key``."""
    import torch
    if torch.is_tensor(key):
        return torch.where(key == 0, torch.full_like(key, -1), 0xFFFFFFFF - (key & 0xFFFFFFFF))
    key = np.asarray(key).astype(np.int64)
    return np.where(key == 0, -1, 0xFFFFFFFF - (key & 0xFFFFFFFF))


def depth_dtype_for(num_z: int) -> np.dtype:
    """The dtype of the unsigned depth plane (z* + 1, 0 = uncovered) of a stack of ``num_z`` levels: uint8 up to 255 levels."""
    if not 1 <= int(num_z) <= 65535:
        raise ValueError(f"a depth plane holds 1..65535 z levels, got {num_z}")
    return np.dtype('uint8') if int(num_z) <= 255 else np.dtype('uint16')


def focus_depth_plane(key, out=None, dtype=None, stream=None):
    """The unsigned depth plane of a key plane of ``fuse_project_focus`` (sq_focus_depth_plane): z* + 1 per voxel, 0 where the
    key is 0 (no plane covers the voxel).  key: [Hc, Wc] device int64 tensor with unit-stride rows.  out: [Hc, Wc] device uint8 /
    uint16 tensor with unit-stride rows, allocated here (``dtype``, default uint8) when None.  Levels the dtype cannot hold
    saturate: size it with ``depth_dtype_for(num_z)``."""
    import torch
    if not torch.is_tensor(key) or key.dtype != torch.int64 or key.dim() != 2:
        raise ValueError("key must be a [Hc, Wc] int64 device tensor")
    shape = tuple(key.shape)
    key_pitch = _check_plane('key', key, shape)
    with _on_stream(stream):
        if out is None:
            out = torch.empty(shape, dtype=torch_dtype_of(np.dtype(dtype or 'uint8')), device=key.device)
        elif dtype is not None and np_dtype_of_torch(out.dtype) != np.dtype(dtype):
            raise ValueError(f"out is {out.dtype}, dtype asks for {np.dtype(dtype)}")
        out_pitch = _check_plane('out', out, shape)
        if out.dtype not in (torch.uint8, torch.uint16):
            raise ValueError("the depth plane is uint8 or uint16")
        h, w = shape
        _check(lib().sq_focus_depth_plane(key.data_ptr(), key_pitch, h, w, out.data_ptr(), out_pitch,
                                          sq_dtype_of(np_dtype_of_torch(out.dtype)), _stream_ptr(stream)), 'sq_focus_depth_plane')
    return out


def fuse_select_depth(plan: FusePlan, tiles, out, depth, z_levels, flats=None, accumulate: bool = False, tile_ptrs=None,
                      flags: int = 0, stream=None, flat_ptrs=None, grid_blocks: int = 0) -> None:
    """A follower channel of the best-focus projection with a guide channel (sq_fuse_select_depth): per voxel
    ``out`` = what ``fuse_planes`` stores there for the plane of this call whose z level is the guide's depth, 0 where the plan
    does not cover the voxel.

    out:      [Hc, Wc] device tensor of the tile dtype with unit-stride rows.
    depth:    [Hc, Wc] device uint8 / uint16 tensor with unit-stride rows: the guide's depth plane (``focus_depth_plane``).
    z_levels: the distinct z levels of the call's Z planes (a sequence, or a device int64 / int32 tensor).
    tiles / tile_ptrs / flats / flat_ptrs: as in ``fuse_project_max`` (Z = tiles.shape[0]; at most 256 planes per call).
    accumulate: voxels whose depth is not among ``z_levels`` are left untouched (the z planes of a channel that come in several
              calls, in any z order, or under different plans); otherwise they are written 0, so every voxel is written."""
    import torch
    if plan.mode != SQ_FUSE_OVERWRITE:
        raise ValueError("fuse_select_depth selects from overwrite plans only")
    shape = (plan.canvas_h, plan.canvas_w)
    pitch = _check_plane('out', out, shape)
    depth_pitch = _check_plane('depth', depth, shape)
    if depth.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("depth must be a uint8 or uint16 tensor")
    n_planes = _projected_planes(plan, tiles, tile_ptrs, flats)
    if not 1 <= n_planes <= SQ_FOCUS_MAX_PLANES:
        raise ValueError(f"{n_planes} planes: a call selects among 1..{SQ_FOCUS_MAX_PLANES}")
    with _on_stream(stream):
        zl = _z_levels_dev(z_levels, n_planes, out.device, distinct=True)
        _fuse_launch('sq_fuse_select_depth', stream, [zl], plan, tiles, n_planes, out, 0, pitch, flats, tile_ptrs, flat_ptrs,
                     depth.data_ptr(), depth_pitch, sq_dtype_of(np_dtype_of_torch(depth.dtype)), zl.data_ptr(),
                     int(flags) | (SQ_SELECT_ACCUMULATE if accumulate else 0), grid_blocks=grid_blocks)


PLANE_ALIGN_BYTES = 128


class _RawDeviceMemory:
    """A range of an arena as an object PyTorch can alias (``__cuda_array_interface__``, uint8); keeps the arena alive."""

    def __init__(self, arena, ptr: int, nbytes: int):
        self._arena = arena
        self.__cuda_array_interface__ = {'shape': (int(nbytes),), 'typestr': '|u1', 'data': (int(ptr), False), 'version': 2}


class DeviceArena:
    """Device memory whose every stretch lies over all memory classes of the card (sq_arena_create, csrc/arena.hip): the
    home of fusion canvases.  An MI355X's memory falls into a few classes of tens of GiB each (thirds of the card where it was scanned); the fusion kernel's
    row-segment writes run at 0.55 of the HBM peak inside one class and at 0.73-0.76 spread over them, and a plain
    allocation gets runs of tens of GiB of ONE class.  The arena takes physical slices, measures their classes and maps them
    round-robin into one virtual range, so a canvas carved from it is fast wherever it starts.

    ``take(nbytes)`` bump-allocates (512-byte aligned) and returns a uint8 tensor aliasing the range; ``reset()`` starts
    over (the caller makes sure nothing uses the old tensors any more); ``close()`` unmaps and releases everything.
    ``natural_order`` (no probe, slices as they come) and ``two_classes`` (the two largest classes only) are the controls of
    A/B measurements."""

    def __init__(self, nbytes: int, device=None, slice_bytes: int = 0, unit_bytes: int = 0, natural_order: bool = False, stream=None,
                 candidate_bytes: Optional[int] = None, two_classes: bool = False):
        import torch
        L = lib()
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        info = _ArenaInfo()
        with torch.cuda.device(self.device):
            if candidate_bytes is None:
                # memory comes in runs of tens of GiB of one class: the call may take what is free (but for a reserve), chunk by
                # chunk, until three classes hold a third of the arena each (after 2.5 x the arena: two classes half each), and
                # gives the rest back (create the arena FIRST, while the card is empty: it then takes 1.5-2.5 times its size; the
                # driver clears what it hands out and what it takes back -- 0.5-6 s for 80 GiB, once per process)
                free = torch.cuda.mem_get_info(self.device)[0]
                candidate_bytes = max(int(nbytes), min(8 * int(nbytes), free - (6 << 30)))
            self._h = L.sq_arena_create(int(nbytes), int(candidate_bytes), int(slice_bytes), int(unit_bytes),
                                        (SQ_ARENA_NATURAL_ORDER if natural_order else 0) | (SQ_ARENA_TWO_CLASSES if two_classes else 0), _stream_ptr(stream), C.byref(info))
        if not self._h:
            raise NativeError(f"sq_arena_create({nbytes} bytes) failed: {L.sq_last_error().decode()}")
        self.base, self.nbytes = int(info.base_dev), int(info.bytes)
        self.info = {'bytes': self.nbytes, 'slice_bytes': int(info.slice_bytes), 'n_slices': int(info.n_slices),
                     'n_candidates': int(info.n_candidates), 'n_classes': int(info.n_classes),
                     'class_slices': [int(v) for v in info.class_slices[:max(1, info.n_classes)]],
                     'class_candidates': [int(v) for v in info.class_candidates[:max(1, info.n_classes)]],
                     'interleaved': bool(info.interleaved), 'probe_ms': round(float(info.probe_ms), 2),
                     'create_ms': round(float(info.create_ms), 1), 'min_pair_gbs': round(float(info.min_pair_gbs), 1),
                     'max_pair_gbs': round(float(info.max_pair_gbs), 1)}
        self._used = 0
        self._holders = []

    def take(self, nbytes: int, align: int = 512):
        """uint8 device tensor of ``nbytes`` bytes at the next ``align``-byte boundary of the arena."""
        import torch
        if not self._h:
            raise NativeError("DeviceArena is closed")
        start = -(-self._used // align) * align
        if start + nbytes > self.nbytes:
            raise NativeError(f"DeviceArena: {nbytes} bytes asked, {self.nbytes - start} of {self.nbytes} left")
        self._used = start + int(nbytes)
        if nbytes == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.device)
        # PyTorch keeps the holder alive for as long as the tensor's STORAGE lives (views included) and nobody else holds it:
        # a weak reference to it says whether the range is still in use
        import weakref
        holder = _RawDeviceMemory(self, self.base + start, nbytes)
        self._holders.append(weakref.ref(holder))
        return torch.as_tensor(holder, device=self.device)

    def in_use(self) -> bool:
        """True while any tensor taken since the last ``reset()`` (or a view of one) is alive."""
        self._holders = [h for h in self._holders if h() is not None]
        return bool(self._holders)

    @property
    def free_bytes(self) -> int:
        return self.nbytes - self._used

    def reset(self) -> None:
        self._used = 0
        self._holders = []

    def close(self) -> None:
        if getattr(self, '_h', None):
            lib().sq_arena_destroy(self._h)      # waits for the device: nothing may be writing into memory that goes away
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def empty_canvas(n_planes: int, hc: int, wc: int, dtype, device, arena: Optional['DeviceArena'] = None):
    """Uninitialised device canvas [n_planes, hc, wc] with dense rows (pitch = wc, like the reference's array)
    whose PLANE stride is rounded up to a multiple of 128 bytes: every plane then starts on a cache-line
    boundary, so the rows of all planes sit at the same phase inside a line and the fusion kernel can carry the
    planes that share a gain image through an item together (fuse.hip, plane groups).  Each plane ``canvas[p]`` is
    contiguous; the tensor as a whole is not.  ``arena``: carve it from this DeviceArena (memory mapped over all
    memory classes of the card: where the fusion kernel writes fastest) instead of a plain allocation."""
    import torch
    esz = torch.empty((), dtype=dtype).element_size()
    unit = PLANE_ALIGN_BYTES // esz
    stride = -(-(hc * wc) // unit) * unit
    if arena is not None:
        flat = arena.take(max(1, n_planes * stride) * esz).view(dtype)
    else:
        flat = torch.empty(max(1, n_planes * stride), dtype=dtype, device=device)
    return flat.as_strided((n_planes, hc, wc), (stride, wc, 1))


def canvas_bytes(n_planes: int, hc: int, wc: int, dtype) -> int:
    """Bytes ``empty_canvas`` takes for this shape (plane stride padded to 128 bytes, start aligned to 512)."""
    import torch
    esz = torch.empty((), dtype=dtype).element_size()
    unit = PLANE_ALIGN_BYTES // esz
    return max(1, n_planes * (-(-(hc * wc) // unit) * unit)) * esz + 512


def planes_to_host(canvas):
    """Device planes [P, Hc, Wc] (any plane stride) -> contiguous numpy array, one D2H copy per plane (a strided
    ``.cpu()`` would first build a contiguous copy ON the device)."""
    import torch
    out = torch.empty(tuple(canvas.shape), dtype=canvas.dtype)
    for p in range(canvas.shape[0]):
        out[p].copy_(canvas[p])
    return out.numpy()


def _tile_table(tiles, tile_ptrs, shape, np_dtype):
    """(ptrs_dev, base_dev, stride, n, h, w, sq dtype, device) for a stack [N, H, W] or a pointer table."""
    if tile_ptrs is not None:
        n = int(tile_ptrs.numel())
        h, w = (int(v) for v in shape)
        return tile_ptrs.data_ptr(), None, 0, n, h, w, sq_dtype_of(np_dtype), tile_ptrs.device
    n, h, w = (int(v) for v in tiles.shape)
    return None, tiles.data_ptr(), h * w, n, h, w, sq_dtype_of(np_dtype_of_torch(tiles.dtype)), tiles.device


def tile_minmax(tiles, stream=None, tile_ptrs=None, shape=None, np_dtype=None):
    """Per-tile (min, max) of a contiguous device stack [N, H, W] (or of the dense H x W tiles a
    device int64 pointer table names) -> device int32 tensor [N, 2] (uint32 on the C side; the
    values fit int32 for uint8/uint16 tiles)."""
    import torch
    L = lib()
    ptrs, base, stride, n, h, w, dt, device = _tile_table(tiles, tile_ptrs, shape, np_dtype)
    with _on_stream(stream):
        out = torch.empty((n, 2), dtype=torch.int32, device=device)
        _check(L.sq_tile_minmax(ptrs, base, stride, n, h, w, w, dt, out.data_ptr(), _stream_ptr(stream)),
               'sq_tile_minmax')
    return out


def pair_overlap_moments(tiles, windows, out=None, stream=None, tile_ptrs=None, shape=None, np_dtype=None):
    """Exact overlap sums of window pairs on a contiguous device stack [N, H, W] (or the dense H x W tiles a device int64
    pointer table names) -> device int64 tensor [n, 5]: sum a, sum b, sum a^2, sum b^2, sum a*b of window pair i, a from
    the reference tile, b from the moving one (uint64 on the C side; every sum of uint16 tiles up to 65535 x 65535 pixels
    stays below 2^63).  ``windows``: OVERLAP_DTYPE records or [n, 8] ints (ref_tile, mov_tile, ref_y0, ref_x0, mov_y0,
    mov_x0, h, w).  ``out``: an int64 [n, 5] device tensor to write into.  A window outside its tile raises NativeError
    and leaves ``out`` as it was.  Reads the window table back to check it, i.e. synchronises the stream.  More than
    OVERLAP_BATCH windows go to the device in batches of that many."""
    import torch
    L = lib()
    ptrs, base, stride, n, h, w, dt, device = _tile_table(tiles, tile_ptrs, shape, np_dtype)
    win = np.asarray(windows)
    if win.dtype != OVERLAP_DTYPE:
        win = np.ascontiguousarray(win, dtype=np.int32).reshape(-1, 8).view(OVERLAP_DTYPE).reshape(-1)
    win = np.ascontiguousarray(win)
    with _on_stream(stream):
        if out is None:
            out = torch.empty((len(win), 5), dtype=torch.int64, device=device)
        if tuple(out.shape) != (len(win), 5) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != device:
            raise ValueError(f"out must be a contiguous int64 [{len(win)}, 5] tensor on {device}")
        if len(win) == 0:
            return out
        win_dev = upload_small(torch.from_numpy(win.view(np.uint8).reshape(-1)), device)
        # the C entry point takes up to OVERLAP_BATCH windows per call (the pair is its grid's y dimension); every window is
        # checked before the first batch is launched, so a bad one still leaves ``out`` untouched
        bad = ((win['ref_tile'] < 0) | (win['ref_tile'] >= n) | (win['mov_tile'] < 0) | (win['mov_tile'] >= n) | (win['h'] < 0)
               | (win['w'] < 0) | (win['ref_y0'] < 0) | (win['ref_x0'] < 0) | (win['mov_y0'] < 0) | (win['mov_x0'] < 0)
               | (win['ref_y0'].astype(np.int64) + win['h'] > h) | (win['mov_y0'].astype(np.int64) + win['h'] > h)
               | (win['ref_x0'].astype(np.int64) + win['w'] > w) | (win['mov_x0'].astype(np.int64) + win['w'] > w))
        if len(win) > OVERLAP_BATCH and bad.any():
            raise NativeError(f"sq_pair_overlap_moments: window {int(np.flatnonzero(bad)[0])} leaves its tile or names no tile")
        for i in range(0, len(win), OVERLAP_BATCH):
            k = min(OVERLAP_BATCH, len(win) - i)
            _check(L.sq_pair_overlap_moments(ptrs, base, stride, n, h, w, w, dt, win_dev.data_ptr() + i * OVERLAP_DTYPE.itemsize, k,
                                             out.data_ptr() + i * 5 * 8, _stream_ptr(stream)), 'sq_pair_overlap_moments')
        if stream is not None:
            win_dev.record_stream(stream)
    return out


def normalize_tiles(tiles, minmax=None, stream=None):
    """normalize_image on a contiguous device stack [N, H, W] -> normalised stack of the same dtype."""
    import torch
    L = lib()
    n, h, w = (int(v) for v in tiles.shape)
    with _on_stream(stream):
        if minmax is None:
            minmax = tile_minmax(tiles, stream)
        out = torch.empty_like(tiles)
        _check(L.sq_normalize_tiles(None, tiles.data_ptr(), h * w, n, h, w, w, sq_dtype_of(np_dtype_of_torch(tiles.dtype)),
                                    minmax.data_ptr(), out.data_ptr(), _stream_ptr(stream)), 'sq_normalize_tiles')
    return out


def _plane_stack(planes, what: str, integer_only: bool):
    """(n, h, w) of a [n, h, w] device tensor with unit-stride rows (any row pitch and plane stride); ValueError otherwise.
    ``integer_only``: uint8 / uint16 only (without it the dtype is left to the entry point, which refuses with NativeError)."""
    import torch
    if planes.dim() != 3 or planes.device.type != 'cuda':
        raise ValueError(f"{what} must be a [n, h, w] device tensor")
    if planes.stride(2) != 1 and planes.shape[2] > 1:
        raise ValueError(f"{what} rows must be contiguous")
    if integer_only and planes.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"{what} must be uint8 or uint16, got {planes.dtype}")
    n, h, w = (int(v) for v in planes.shape)
    return n, h, w


def _check_out_stack(out, shape, like) -> None:
    """``out`` is a stack of this shape with the dtype and device of ``like`` and unit-stride rows; ValueError otherwise."""
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device:
        raise ValueError(f"out must be a {tuple(shape)} tensor of the input's dtype and device")
    if out.numel() and out.stride(2) != 1 and out.shape[2] > 1:
        raise ValueError("out rows must be contiguous")


def downsample2(planes, out=None, stream=None):
    """Next pyramid level of ``planes`` [n, h, w] (uint8 / uint16 device tensor, any row pitch) ->
    [n, h // 2, w // 2]: out[p, y, x] = planes[p, 2y+1, 2x+1], what ome_zarr's Scaler.nearest computes per
    level (stitcher.py:797-798).  ``out`` may be a preallocated tensor (any row pitch)."""
    import torch
    L = lib()
    n, h, w = _plane_stack(planes, 'planes', integer_only=False)
    with _on_stream(stream):
        if out is None:
            out = torch.empty((n, h // 2, w // 2), dtype=planes.dtype, device=planes.device)
        _check_out_stack(out, (n, h // 2, w // 2), planes)
        if out.numel() == 0:
            return out
        _check(L.sq_downsample2(planes.data_ptr(), planes.stride(0), h, w, planes.stride(1), out.data_ptr(), out.stride(0),
                                out.stride(1), n, sq_dtype_of(np_dtype_of_torch(planes.dtype)), _stream_ptr(stream)),
               'sq_downsample2')
    return out


SQ_PYRAMID_MEAN_MAX_LEVELS = 5     # levels one sq_pyramid_mean launch yields (squidstitch.h); longer requests take further launches


def pyramid_mean(planes, n_levels, out=None, stream=None):
    """The next ``n_levels`` MEAN pyramid levels of ``planes`` [n, h, w] (uint8 / uint16 device tensor, any row pitch) from
    one read of it -> list of [n, h >> l, w >> l], l = 1 ... : every level is the truncated 2 x 2 mean of the level before,
    ``(a + b + c + d) >> 2``, a trailing odd row / column dropped (what the reference's zarr_stitcher.py:614-719 stores:
    ``da.coarsen(np.mean, ..., trim_excess=True)`` cast to the integer dtype).  Levels that would be empty are not returned.
    ``out`` may be a list of preallocated tensors (any row pitch), one per level that exists."""
    import torch
    L = lib()
    n, h, w = _plane_stack(planes, 'planes', integer_only=True)
    dtype = sq_dtype_of(np_dtype_of_torch(planes.dtype))
    n_levels = int(n_levels)
    if n_levels < 0:
        raise ValueError(f"n_levels must be >= 0, got {n_levels}")
    shapes = []
    while len(shapes) < n_levels and (h >> (len(shapes) + 1)) > 0 and (w >> (len(shapes) + 1)) > 0:
        shapes.append((n, h >> (len(shapes) + 1), w >> (len(shapes) + 1)))
    with _on_stream(stream):
        if out is None:
            out = [torch.empty(s, dtype=planes.dtype, device=planes.device) for s in shapes]
        out = list(out)
        if len(out) != len(shapes):
            raise ValueError(f"out must hold {len(shapes)} tensors (the levels of a {(n, h, w)} stack that exist), got {len(out)}")
        for s, o in zip(shapes, out):
            _check_out_stack(o, s, planes)
        if not shapes or n == 0:
            return out
        k = len(shapes)
        ptrs = (C.c_void_p * k)(*[o.data_ptr() for o in out])
        strides = (C.c_int64 * k)(*[o.stride(0) for o in out])
        pitches = (C.c_int64 * k)(*[o.stride(1) for o in out])
        _check(L.sq_pyramid_mean(planes.data_ptr(), planes.stride(0), h, w, planes.stride(1), ptrs, strides, pitches, k, n, dtype,
                                 _stream_ptr(stream)), 'sq_pyramid_mean')
    return out


def histogram_bins(dtype) -> int:
    """Bins of a histogram row of this dtype (one per value): 256 for uint8, 65536 for uint16."""
    dt = np.dtype(dtype)
    if dt not in (np.dtype('uint8'), np.dtype('uint16')):
        raise ValueError(f"histograms are kept for uint8 and uint16 planes, got {dt}")
    return 1 << (8 * dt.itemsize)


def histogram_planes(planes, rows, hist=None, n_rows=None, stream=None):
    """Exact value counts of ``planes`` [n, h, w] (uint8 / uint16 device tensor, any row pitch) ADDED into ``hist``, an int64
    device tensor [n_rows, bins] (bins = 256 / 65536): ``hist[rows[p], v] += count of v in planes[p]``.  ``rows``: one int per
    plane, 0 <= row < n_rows (several planes may share a row).  ``hist`` None: a zeroed [n_rows, bins] tensor is made
    (n_rows None: max(rows) + 1).  Returns ``hist``.  The reference has no counterpart (its channel windows are
    np.iinfo(dtype).max, stitcher.py:846-850); the definition is numpy.bincount."""
    import torch
    L = lib()
    n, h, w = _plane_stack(planes, 'planes', integer_only=True)
    np_dtype = np_dtype_of_torch(planes.dtype)
    bins = histogram_bins(np_dtype)
    rows = [int(r) for r in rows]
    if len(rows) != n:
        raise ValueError(f"{n} planes, {len(rows)} rows given")
    with _on_stream(stream):
        if hist is None:
            if n_rows is None:
                n_rows = max(rows) + 1 if rows else 1
            hist = torch.zeros((int(n_rows), bins), dtype=torch.int64, device=planes.device)
        if hist.dim() != 2 or hist.shape[1] != bins or hist.dtype != torch.int64 or hist.device != planes.device or \
                not hist.is_contiguous():
            raise ValueError(f"hist must be a contiguous int64 [n_rows, {bins}] tensor on the planes' device")
        if n_rows is not None and int(n_rows) != hist.shape[0]:
            raise ValueError(f"hist has {hist.shape[0]} rows, n_rows = {n_rows}")
        if n == 0 or h == 0 or w == 0:
            if any(not 0 <= r < hist.shape[0] for r in rows):
                raise ValueError(f"rows must lie in [0, {hist.shape[0]})")
            return hist
        table = (C.c_int32 * n)(*rows) if all(-2 ** 31 <= r < 2 ** 31 for r in rows) else None
        if table is None:
            raise ValueError(f"rows must lie in [0, {hist.shape[0]})")
        _check(L.sq_histogram_planes(planes.data_ptr(), planes.stride(0), h, w, planes.stride(1), n, sq_dtype_of(np_dtype), table,
                                     int(hist.shape[0]), hist.data_ptr(), _stream_ptr(stream)), 'sq_histogram_planes')
    return hist


SQ_BLOCK_MEAN_MAX_K = 8            # block sums of uint16 values fit 32 bits up to 256 x 256 (squidstitch.h)
SQ_COMPOSITE_MAX_PLANES = 16


def block_mean(planes, k, out=None, rows=None, stream=None):
    """Block means of ``planes`` [n, H, W] (uint8 / uint16 device tensor, any row pitch) -> [n, ceil(H / f), ceil(W / f)] of the
    same dtype, f = 2^k, k = 0 ... 8: the truncated mean of every f x f block over the pixels of it that exist (partial blocks
    at the bottom and right edge; k = 0 is the identity).  Replaces the host copy of stitcher.py:861-885 (_save_debug_slice);
    the definition is ``tests/composite_ref.block_mean``.  ``rows`` = (y0, y1): only source rows [y0, y1) are read and rows
    y0 / f ... of ``out`` written (y0 a multiple of f, y1 - y0 a multiple of f or y1 = H) -- what a rank that wrote a row band
    reduces.  ``out`` may be a preallocated tensor (any row pitch); without it a fresh one is made (zeroed when ``rows`` leaves
    part of it unwritten)."""
    import torch
    L = lib()
    n, h, w = _plane_stack(planes, 'planes', integer_only=True)
    k = int(k)
    if not 0 <= k <= SQ_BLOCK_MEAN_MAX_K:
        raise ValueError(f"k must lie in 0..{SQ_BLOCK_MEAN_MAX_K}, got {k}")
    f = 1 << k
    shape = (n, -(-h // f), -(-w // f))
    y0, y1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if not (0 <= y0 <= y1 <= h) or y0 % f or ((y1 - y0) % f and y1 != h):
        raise ValueError(f"rows {rows} of {h}: a band starts on a multiple of {f} and is a multiple of it long, or runs to the last row")
    with _on_stream(stream):
        if out is None:
            out = (torch.empty if (y0, y1) == (0, h) else torch.zeros)(shape, dtype=planes.dtype, device=planes.device)
        _check_out_stack(out, shape, planes)
        if n == 0 or h == 0 or w == 0 or y1 == y0:
            return out
        _check(L.sq_block_mean(planes.data_ptr(), planes.stride(0), h, w, planes.stride(1), n, sq_dtype_of(np_dtype_of_torch(planes.dtype)),
                               k, y0, y1 - y0, out.data_ptr(), out.stride(0), out.stride(1), _stream_ptr(stream)), 'sq_block_mean')
    return out


def composite_render(means, windows, colors, out=None, stream=None):
    """``means`` [n, h, w] (uint8 / uint16 device tensor, n <= 16, any row pitch), one window (start, end) and one colour
    0xRRGGBB per plane -> interleaved RGB8 [h, w, 3] on the device: every plane is mapped through its window to 0 ... 255
    (0 at or below start, 255 at or above end, floor((m - start) * 255 / (end - start)) between), scaled by its colour
    (floor(v * component / 255)) and the planes are added, saturating at 255.  Replaces the min/max normalisation of
    stitcher.py:861-885 (_save_debug_slice); the definition is ``tests/composite_ref.render``.  ``out``: a preallocated uint8
    [h, w, 3] tensor whose pixels are contiguous (any row pitch)."""
    import torch
    L = lib()
    n, h, w = _plane_stack(means, 'means', integer_only=True)
    if not 1 <= n <= SQ_COMPOSITE_MAX_PLANES:
        raise ValueError(f"1..{SQ_COMPOSITE_MAX_PLANES} planes, got {n}")
    windows = [(int(a), int(b)) for a, b in windows]
    colors = [int(c) for c in colors]
    if len(windows) != n or len(colors) != n:
        raise ValueError(f"{n} planes, {len(windows)} windows and {len(colors)} colours given")
    if any(not 0 <= a < b <= 65535 for a, b in windows):
        raise ValueError(f"windows must satisfy 0 <= start < end <= 65535, got {windows}")
    if any(not 0 <= c <= 0xFFFFFF for c in colors):
        raise ValueError(f"colours are 0xRRGGBB, got {colors}")
    with _on_stream(stream):
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=means.device)
        if tuple(out.shape) != (h, w, 3) or out.dtype != torch.uint8 or out.device != means.device:
            raise ValueError(f"out must be a uint8 {(h, w, 3)} tensor on the planes' device")
        if out.numel() and (out.stride(2) != 1 or out.stride(1) != 3):
            raise ValueError("out pixels must be contiguous (strides (pitch, 3, 1))")
        if h == 0 or w == 0:
            return out
        win = (C.c_int32 * (2 * n))(*[v for ab in windows for v in ab])
        col = (C.c_uint32 * n)(*colors)
        _check(L.sq_composite_render(means.data_ptr(), means.stride(0), h, w, means.stride(1), n,
                                     sq_dtype_of(np_dtype_of_torch(means.dtype)), win, col, out.data_ptr(), out.stride(0),
                                     _stream_ptr(stream)), 'sq_composite_render')
    return out


SQ_TOPHAT_MAX_RADIUS = 127


def tophat_scratch_bytes(n_images: int, h: int, w: int, dtype) -> int:
    """Bytes of the caller-owned scratch of ``tophat_tiles`` for ``n_images`` planes of h x w (uint8 / uint16): the erosion of
    the batch, as many bytes as the planes themselves."""
    dt = np.dtype(dtype)
    if dt not in (np.dtype('uint8'), np.dtype('uint16')):
        raise ValueError(f"the top-hat filters uint8 and uint16 planes, got {dt}")
    if int(n_images) < 0 or int(h) < 1 or int(w) < 1:
        raise ValueError(f"bad sizes: {n_images} planes of {h} x {w}")
    return _size(lib().sq_tophat_scratch_bytes(int(n_images), int(h), int(w), sq_dtype_of(dt)), 'sq_tophat_scratch_bytes')


def tophat_tiles(tiles, radius: int, scratch=None, stream=None):
    """White top-hat of every H x W plane of ``tiles`` IN PLACE (sq_tophat_tiles; an extension, the reference has none): the plane
    minus its morphological opening with a square (2R+1) x (2R+1) window clipped to the plane -- ``tests/tophat_ref.tophat``.

    tiles:   a plane batch (``_plane_batch``).
    radius:  R, 1..127 (windows larger than the plane are fine).
    scratch: optional device uint8 tensor of at least ``tophat_scratch_bytes(n_planes, H, W, dtype)`` bytes (reuse it across
             calls); allocated here when None.
    Returns ``tiles``."""
    import torch
    n_images, h, w, plane_stride, pitch = _plane_batch(tiles, 'tiles')
    radius = _int_in(radius, 1, SQ_TOPHAT_MAX_RADIUS, 'top-hat radius')
    np_dtype = np_dtype_of_torch(tiles.dtype)
    need = tophat_scratch_bytes(n_images, h, w, np_dtype)
    with _on_stream(stream):
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.uint8, device=tiles.device)
            if stream is not None:
                scratch.record_stream(stream)
        elif not torch.is_tensor(scratch) or not scratch.is_cuda or not scratch.is_contiguous() or \
                scratch.numel() * scratch.element_size() < need:
            raise ValueError(f"top-hat scratch must be a contiguous device tensor of at least {need} bytes")
        if scratch.data_ptr() % 16:
            raise ValueError("top-hat scratch must be aligned to 16 bytes")
        if n_images == 0:
            return tiles
        _check(lib().sq_tophat_tiles(tiles.data_ptr(), n_images, h, w, plane_stride, pitch, sq_dtype_of(np_dtype), int(radius),
                                     scratch.data_ptr(), scratch.numel() * scratch.element_size(), _stream_ptr(stream)),
               'sq_tophat_tiles')
    return tiles


SQ_DESPECKLE_HOT = 1
SQ_DESPECKLE_BOTH = 2
DESPECKLE_MODES = {'hot': SQ_DESPECKLE_HOT, 'both': SQ_DESPECKLE_BOTH}
SQ_DESPECKLE_MAX_THRESHOLD = 65535


def _plane_layout(t, what):
    """(n_planes, h, w, plane stride, pitch) of a [..., H, W] tensor with unit-stride rows whose leading dimensions are one
    uniform plane stride apart (elements); ValueError otherwise."""
    h, w = int(t.shape[-2]), int(t.shape[-1])
    if h < 1 or w < 1:
        raise ValueError(f"{what}: planes of {h} x {w}")
    if w > 1 and t.stride(-1) != 1:
        raise ValueError(f"{what} rows must be contiguous")
    pitch = int(t.stride(-2)) if h > 1 else w
    if pitch < w:
        raise ValueError(f"{what} rows overlap")
    lead = [(int(n), int(s)) for n, s in zip(t.shape[:-2], t.stride()[:-2]) if n != 1]
    n_images = 1
    for n, _ in lead:
        n_images *= n
    plane_stride = (h - 1) * pitch + w
    if n_images > 1:
        for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
            if s0 != n1 * s1:
                raise ValueError(f"the planes of {what} must be a uniform stride apart (a contiguous stack or a regular view "
                                 "of one)")
        plane_stride = lead[-1][1]
        if plane_stride < (h - 1) * pitch + w:
            raise ValueError(f"the planes of {what} overlap")
    return n_images, h, w, plane_stride, pitch


def _byte_extent(t, layout):
    """(first byte, one past the last byte) of the planes of ``t``, ``layout`` its ``_plane_layout`` with at least one plane:
    the whole range the run spans, the gaps between its rows and planes included."""
    n_images, h, w, plane_stride, pitch = layout
    first = t.data_ptr()
    return first, first + ((n_images - 1) * plane_stride + (h - 1) * pitch + w) * t.element_size()


def _overlap(a, b) -> bool:
    """Two byte extents share memory (interleaved views such as t[::2] and t[1::2] count: their ranges do)."""
    return a[0] < b[1] and b[0] < a[1]


def _plane_batch(t, name, shape='[..., H, W]', dims=None):
    """The plane batch every per-tile filter takes: ``t`` is a uint8 / uint16 device tensor [..., H, W] with unit-stride rows
    (any row pitch, any base offset) whose leading dimensions are one uniform plane stride apart -- a contiguous stack, or a
    view such as every other plane of one.  -> its ``_plane_layout``; ValueError otherwise."""
    import torch
    if not torch.is_tensor(t) or not t.is_cuda or (t.dim() < 2 if dims is None else t.dim() not in dims):
        raise ValueError(f"{name} must be a {shape} device tensor")
    if t.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"{name} must be uint8 or uint16, got {t.dtype}")
    return _plane_layout(t, name)


def _out_of_place(out, shape, tiles, src, noun, stream):
    """The ``out`` of an out-of-place filter of the plane batch ``tiles`` (``src`` its layout), inside ``_on_stream(stream)``:
    allocated contiguous when None, else a tensor of ``shape`` with the tiles' dtype and device that is a plane batch itself (its
    columns beyond W stay as they are) and whose byte extent does not meet the tiles'.  -> (out, its layout)."""
    import torch
    if out is None:
        out = torch.empty(shape, dtype=tiles.dtype, device=tiles.device)
        if stream is not None:
            out.record_stream(stream)
    elif not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != tiles.dtype or out.device != tiles.device:
        raise ValueError(f"out must be a {tiles.dtype} tensor of shape {shape} on the tiles' device")
    dst = _plane_layout(out, 'out')
    assert dst[0] == src[0]
    if src[0] and _overlap(_byte_extent(tiles, src), _byte_extent(out, dst)):
        raise ValueError(f"out shares memory with tiles: the {noun} is out of place")
    return out, dst


def _tuple_table(values, tiles, ranges, name, entry):
    """``values`` is one tuple of integers for every plane of ``tiles``, or a sequence of one tuple per index of the leading
    dimension (all planes under that index take it); position i of a tuple lies in ``ranges[i]`` = (lo, hi, noun).
    -> (the flat int32 table for the library, the number of tuples); ``name`` and ``entry`` word the refusals."""
    width = len(ranges)
    try:
        entries = list(values)
    except TypeError:
        raise ValueError(f"{name} must be {entry} or a sequence of them, got {values!r}")
    if len(entries) == width and not any(isinstance(v, (list, tuple, np.ndarray)) for v in entries):
        entries = [entries]      # one tuple for every plane
    elif tiles.dim() < 3 or len(entries) != tiles.shape[0]:
        raise ValueError(f"{name} must be {entry}, or one per index of the leading dimension "
                         f"({tiles.shape[0] if tiles.dim() > 2 else 1}), got {len(entries)}")
    table = []
    for e in entries:
        if isinstance(e, (str, bytes)) or not hasattr(e, '__len__') or len(e) != width:
            raise ValueError(f"an entry of {name} is {entry}, got {e!r}")
        table += [_int_in(v, lo, hi, noun) for v, (lo, hi, noun) in zip(e, ranges)]
    return (C.c_int32 * len(table))(*table), len(entries)


def despeckle_tiles(tiles, threshold: int, mode: str = 'hot', out=None, counts=None, stream=None):
    """Hot-pixel removal of every H x W plane of ``tiles`` into ``out`` (sq_despeckle_tiles; an extension, the reference has
    none): a pixel that differs from the median m of its edge-replicated 3 x 3 window by more than ``threshold`` -- mode 'hot':
    I - m > T; mode 'both': |I - m| > T -- is replaced by m, every m taken from the unfiltered plane --
    ``tests/despeckle_ref.despeckle``.  The filter is out of place: ``tiles`` is left as it is and the caller goes on with the
    return value.

    tiles:     a plane batch (``_plane_batch``).
    threshold: T, an integer in 0..65535, in counts of the planes' dtype.
    out:       a tensor of the same shape, dtype and device under the same rules (its columns beyond W stay as they are) that
               shares no memory with ``tiles``; allocated contiguous when None.
    counts:    optional contiguous int64 device tensor with one element per plane: the number of pixels replaced in each plane
               is ADDED to it.
    Returns ``out``."""
    import torch
    src = _plane_batch(tiles, 'tiles')
    n_images, h, w, src_plane_stride, src_pitch = src
    threshold = _int_in(threshold, 0, SQ_DESPECKLE_MAX_THRESHOLD, 'despeckle threshold')
    if not isinstance(mode, str) or mode not in DESPECKLE_MODES:
        raise ValueError(f"despeckle mode must be 'hot' or 'both', got {mode!r}")
    with _on_stream(stream):
        out, (_, _, _, dst_plane_stride, dst_pitch) = _out_of_place(out, tuple(tiles.shape), tiles, src, 'filter', stream)
        if counts is not None:
            if not torch.is_tensor(counts) or counts.dtype != torch.int64 or counts.device != tiles.device or \
                    counts.numel() != n_images or not counts.is_contiguous():
                raise ValueError(f"counts must be a contiguous int64 tensor of {n_images} elements on the tiles' device")
        if n_images == 0:
            return out
        _check(lib().sq_despeckle_tiles(tiles.data_ptr(), out.data_ptr(), n_images, h, w, src_plane_stride, src_pitch,
                                        dst_plane_stride, dst_pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)),
                                        DESPECKLE_MODES[mode], threshold,
                                        None if counts is None else counts.data_ptr(), _stream_ptr(stream)),
               'sq_despeckle_tiles')
    return out


SQ_TILE_STATS_WORDS = 8
SQ_TILE_STATS_ROWS_PER_THREAD = 64      # rows one thread of the kernel walks down (include/squidstitch.h): the tests' sizes


def tile_stats(tiles, out=None, stream=None):
    """The eight quality words of every H x W plane of ``tiles`` (sq_tile_stats; an extension, the reference has none): min,
    max, sum, sum of squares, pixels at the dtype's maximum, pixels at 0 and the Brenner sums with step 2 along x and along y
    -- ``tests/tile_qc_ref.tile_words``; ``tileqc.derive`` makes mean, std, focus and the saturated fraction of them.

    tiles: uint8 / uint16 device tensor [n, H, W] or [b, n, H, W] with unit-stride rows (any row pitch, any base offset) whose
           leading dimensions collapse to one plane stride (at least a plane); anything else raises ValueError.
    out:   int64 device tensor [planes, 8]; its words are overwritten.  Allocated when None.
    Returns ``out``."""
    import torch
    n_images, h, w, plane_stride, pitch = _plane_batch(tiles, 'tiles', '[n, H, W] or [b, n, H, W]', (3, 4))
    with _on_stream(stream):
        if out is None:
            out = torch.empty((n_images, SQ_TILE_STATS_WORDS), dtype=torch.int64, device=tiles.device)
            if stream is not None:
                out.record_stream(stream)
        elif not torch.is_tensor(out) or out.dtype != torch.int64 or out.device != tiles.device or \
                tuple(out.shape) != (n_images, SQ_TILE_STATS_WORDS) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 tensor of shape ({n_images}, {SQ_TILE_STATS_WORDS}) on the tiles' device")
        if n_images == 0:
            return out
        _check(lib().sq_tile_stats(tiles.data_ptr(), n_images, h, w, plane_stride, pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)),
                                   out.data_ptr(), _stream_ptr(stream)), 'sq_tile_stats')
    return out


SQ_SEAM_MAX_RADIUS = 3


def seam_words(radius: int) -> int:
    """Words per (plane, seam) of sq_seam_stats at search radius R: Sa, Saa, Sad and (Sb, Sbb, Sab) of (2R + 1)^2 offsets."""
    radius = _int_in(radius, 0, SQ_SEAM_MAX_RADIUS, 'seam radius')
    return 3 + 3 * (2 * radius + 1) ** 2


def as_overlaps(pairs) -> np.ndarray:
    """OVERLAP_DTYPE records, or [n, 8] ints (ref_tile, mov_tile, ref_y0, ref_x0, mov_y0, mov_x0, h, w) -> contiguous
    OVERLAP_DTYPE [n]; ValueError for anything else."""
    win = np.asarray(pairs)
    if win.dtype != OVERLAP_DTYPE:
        if win.dtype.kind not in 'iu' or (win.size and (win.ndim != 2 or win.shape[1] != 8)):
            raise ValueError("pairs must be OVERLAP_DTYPE records or an [n, 8] integer array")
        if win.size and (np.abs(win.astype(np.int64)) >= 2 ** 31).any():
            raise ValueError("a pair's coordinate does not fit int32")
        win = np.ascontiguousarray(win, dtype=np.int32).reshape(-1, 8).view(OVERLAP_DTYPE)
    return np.ascontiguousarray(win.reshape(-1))


def seam_pairs_to_device(pairs, device):
    """The device copy of a pair table that ``seam_stats`` takes as ``pairs_dev`` (a caller with one table for many calls
    uploads it once)."""
    import torch
    return upload_small(torch.from_numpy(as_overlaps(pairs).view(np.uint8).reshape(-1).copy()), device)


def seam_stats(tiles, pairs, radius, out=None, stream=None, pairs_dev=None):
    """The alignment words of every (plane, pair) of ``tiles`` (sq_seam_stats; an extension, the reference has none): for the
    core windows a(y, x) of the ref tile and b_e(y, x) = mov[my + y - ey, mx + x - ex] of the mov tile, Sa, Saa, Sad = sum
    |a - b_0| and then, row-major over e = (ey, ex) in [-R, R]^2, Sb_e, Sbb_e, Sab_e -- ``tests/seam_qc_ref.pair_words``;
    ``seamqc.derive`` makes the ncc at the placement, the best residual displacement and the flags of them.

    tiles:  uint8 / uint16 device tensor [m, n, H, W]: m planes of n tiles with unit-stride rows (any row pitch, any base
            offset), the tiles one stride apart and the planes another; anything else raises ValueError.
    pairs:  host array of OVERLAP_DTYPE records (or [k, 8] ints): the core windows at e = 0, the same for every plane.  A
            tile index outside 0..n-1, a ref window outside its tile or a mov window nearer than R to an edge of its tile raises
            NativeError, and nothing is launched.
    radius: R, an integer in 0..SQ_SEAM_MAX_RADIUS.
    out:    contiguous int64 device tensor [m, k, seam_words(R)]; its words are overwritten.  Allocated when None.
    pairs_dev: ``seam_pairs_to_device(pairs, device)`` kept from an earlier call with the same table; uploaded here when None.
    Returns ``out``."""
    import torch
    if not torch.is_tensor(tiles) or not tiles.is_cuda or tiles.dim() != 4:
        raise ValueError("tiles must be a [m, n, H, W] device tensor")
    if tiles.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"tiles must be uint8 or uint16, got {tiles.dtype}")
    words = seam_words(radius)
    win = as_overlaps(pairs)
    m, n = int(tiles.shape[0]), int(tiles.shape[1])
    if m and n:
        _, h, w, tile_stride, pitch = _plane_layout(tiles[0], 'tiles')
        plane_stride = int(tiles.stride(0)) if m > 1 else (n - 1) * tile_stride + (h - 1) * pitch + w
        if plane_stride < (n - 1) * tile_stride + (h - 1) * pitch + w:
            raise ValueError("the planes of tiles overlap")
    else:
        h, w = int(tiles.shape[2]), int(tiles.shape[3])
        if h < 1 or w < 1:
            raise ValueError(f"tiles: planes of {h} x {w}")
        tile_stride, pitch, plane_stride = h * w, w, n * h * w
    with _on_stream(stream):
        if out is None:
            out = torch.empty((m, len(win), words), dtype=torch.int64, device=tiles.device)
            if stream is not None:
                out.record_stream(stream)
        elif not torch.is_tensor(out) or out.dtype != torch.int64 or out.device != tiles.device or \
                tuple(out.shape) != (m, len(win), words) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 tensor of shape ({m}, {len(win)}, {words}) on the tiles' device")
        if m == 0 or len(win) == 0:
            return out
        if n == 0:
            raise NativeError(f"sq_seam_stats: {len(win)} pairs of no tiles")
        if pairs_dev is None:
            pairs_dev = seam_pairs_to_device(win, tiles.device)
        elif not torch.is_tensor(pairs_dev) or pairs_dev.device != tiles.device or pairs_dev.dtype != torch.uint8 or \
                pairs_dev.numel() != win.nbytes or not pairs_dev.is_contiguous():
            raise ValueError("pairs_dev must be seam_pairs_to_device(pairs, device) of the same table")
        _check(lib().sq_seam_stats(tiles.data_ptr(), m, n, h, w, plane_stride, tile_stride, pitch,
                                   sq_dtype_of(np_dtype_of_torch(tiles.dtype)), win.ctypes.data, pairs_dev.data_ptr(), len(win),
                                   radius, out.data_ptr(), _stream_ptr(stream)), 'sq_seam_stats')
        pairs_dev.record_stream(torch.cuda.current_stream(tiles.device))      # (the stream of the launch, inside _on_stream)
    return out


SQ_DPC_MAX_GAIN = 16
DPC_CHANNEL = 'DPC'      # the derived channel's name (stitcher.py)
DPC_DEFINITION = 'S = L + R; N = S + 2*gain*(L - R); DPC = 0 if S == 0 else clamp(floor(M*N / (2*S)), 0, M), M = the dtype maximum'


def dpc_tiles(left, right, gain: int = 1, out=None, stream=None):
    """Differential phase contrast of every H x W plane of ``left`` and ``right`` (sq_dpc_tiles; an extension, the reference
    has none): with S = L + R, N = S + 2 gain (L - R) and M the dtype's maximum, 0 where S == 0 and
    clamp(floor(M N / (2 S)), 0, M) elsewhere, exact in integers -- ``tests/dpc_ref.dpc_image``.

    left, right: uint8 / uint16 device tensors [..., H, W] of one dtype and shape with unit-stride rows (any row pitch) whose
                 leading dimensions are one uniform plane stride apart, each with its own.
    gain:        an integer in 1..16.
    out:         None: in place over ``left``.  Else a tensor of the same shape, dtype and device under the same rules (its
                 columns beyond W stay as they are) that is exactly ``left`` or shares no memory with either input.
    Returns ``out`` (``left`` when None)."""
    import torch
    lay_l = _plane_batch(left, 'left')
    gain = _int_in(gain, 1, SQ_DPC_MAX_GAIN, 'dpc gain')
    if out is None:
        out = left
    for name, t in (('right', right), ('out', out)):
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(left.shape) or t.dtype != left.dtype or t.device != left.device:
            raise ValueError(f"{name} must be a {left.dtype} tensor of shape {tuple(left.shape)} on left's device")
    lay_r, lay_o = _plane_layout(right, 'right'), _plane_layout(out, 'out')
    n_images, h, w, left_plane_stride, left_pitch = lay_l
    (right_plane_stride, right_pitch), (out_plane_stride, out_pitch) = lay_r[3:], lay_o[3:]
    if n_images == 0:
        return out
    ext_l, ext_r, ext_o = _byte_extent(left, lay_l), _byte_extent(right, lay_r), _byte_extent(out, lay_o)
    in_place = ext_o[0] == ext_l[0] and out_pitch == left_pitch and (n_images == 1 or out_plane_stride == left_plane_stride)
    if (not in_place and _overlap(ext_l, ext_o)) or _overlap(ext_r, ext_o):
        raise ValueError("out must be exactly left (in place) or share no memory with left and right")
    _check(lib().sq_dpc_tiles(left.data_ptr(), right.data_ptr(), out.data_ptr(), n_images, h, w, left_plane_stride, left_pitch,
                              right_plane_stride, right_pitch, out_plane_stride, out_pitch,
                              sq_dtype_of(np_dtype_of_torch(left.dtype)), gain, _stream_ptr(stream)), 'sq_dpc_tiles')
    return out


SQ_BIN_MEAN = 1
SQ_BIN_SUM = 2
SQ_BIN_MAX_FACTOR = 8
BIN_METHODS = {'mean': SQ_BIN_MEAN, 'sum': SQ_BIN_SUM}


def bin_tiles(tiles, factor: int, method: str = 'mean', out=None, stream=None):
    """K x K binning of every H x W plane of ``tiles`` into ``out`` (sq_bin_tiles; an extension, the reference has nothing
    like it): with hb = H // K and wb = W // K -- the last H - K hb rows and W - K wb columns are dropped -- and S the sum of
    a K x K block, 'mean' gives floor(S / K^2) and 'sum' gives min(S, M), M the dtype's maximum, exact in integers --
    ``tests/bin_ref.bin_image``.  The binning is out of place: ``tiles`` is left as it is.

    tiles:  a plane batch (``_plane_batch``).
    factor: K, an integer in 2..8 no larger than H or W.
    method: 'mean' or 'sum'.
    out:    a tensor [..., hb, wb] with the same leading dimensions, dtype and device under the same rules (its columns beyond
            wb stay as they are) that shares no memory with ``tiles``; allocated contiguous when None.
    Returns ``out``."""
    import torch
    factor = _int_in(factor, 2, SQ_BIN_MAX_FACTOR, 'binning factor')
    if not isinstance(method, str) or method not in BIN_METHODS:
        raise ValueError(f"binning method must be 'mean' or 'sum', got {method!r}")
    src = _plane_batch(tiles, 'tiles')
    n_images, h, w, src_plane_stride, src_pitch = src
    hb, wb = h // factor, w // factor
    if hb < 1 or wb < 1:
        raise ValueError(f"planes of {h} x {w} have no {factor} x {factor} block")
    with _on_stream(stream):
        out, (_, _, _, dst_plane_stride, dst_pitch) = _out_of_place(out, tuple(tiles.shape[:-2]) + (hb, wb), tiles, src, 'binning', stream)
        if n_images == 0:
            return out
        _check(lib().sq_bin_tiles(tiles.data_ptr(), out.data_ptr(), n_images, h, w, src_plane_stride, src_pitch,
                                  dst_plane_stride, dst_pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)), factor,
                                  BIN_METHODS[method], _stream_ptr(stream)), 'sq_bin_tiles')
    return out


SQ_WARP_MAX_PPM = 50000
SQ_WARP_MAX_SIDE = 65535
SQ_WARP_PLANES_PER_THREAD = 16


def warp_tiles(tiles, ppm: int, out=None, stream=None):
    """Radial lens correction of every H x W plane of ``tiles`` into ``out`` (sq_warp_tiles; an extension, the reference has
    nothing like it): the output at radius r takes the input at radius r (1 + ppm 10^-6 r^2 / R^2), R the plane's half
    diagonal, bilinearly with 8 fractional bits and replicated edges, exact in integers -- ``tests/warp_ref.warp_image``; the
    formula stands in include/squidstitch.h.  The correction is out of place: ``tiles`` is left as it is.

    tiles:  a plane batch (``_plane_batch``), H and W at most 65535.
    ppm:    an integer in -50000..50000, the relative displacement at the plane's corner in parts per million; positive
            undoes pincushion, negative barrel distortion, 0 gives an exact copy.
    out:    None, or the tensor to fill: ``_out_of_place``.
    Returns ``out``."""
    import torch
    ppm = _int_in(ppm, -SQ_WARP_MAX_PPM, SQ_WARP_MAX_PPM, 'distortion ppm')
    src = _plane_batch(tiles, 'tiles')
    n_images, h, w, src_plane_stride, src_pitch = src
    if h > SQ_WARP_MAX_SIDE or w > SQ_WARP_MAX_SIDE:
        raise ValueError(f"planes of {h} x {w} have a side above {SQ_WARP_MAX_SIDE}")
    with _on_stream(stream):
        out, (_, _, _, dst_plane_stride, dst_pitch) = _out_of_place(out, tuple(tiles.shape), tiles, src, 'correction', stream)
        if n_images == 0:
            return out
        _check(lib().sq_warp_tiles(tiles.data_ptr(), out.data_ptr(), n_images, h, w, src_plane_stride, src_pitch,
                                   dst_plane_stride, dst_pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)), ppm,
                                   _stream_ptr(stream)), 'sq_warp_tiles')
    return out


SQ_SHIFT_MAX = 16384
SQ_SHIFT_MAX_SIDE = 65535
SQ_SHIFT_ROWS_PER_THREAD = 32


def shift_tiles(tiles, shifts, out=None, stream=None):
    """Constant sub-pixel translation of every H x W plane of ``tiles`` into ``out`` (sq_shift_tiles; an extension, the
    reference has nothing like it): the output at (y, x) takes the input at (y + Sy/256, x + Sx/256), bilinearly with 8
    fractional bits and replicated edges, exact in integers -- ``tests/shift_ref.shift_image``; the formula stands in
    include/squidstitch.h.  The shift is out of place: ``tiles`` is left as it is.

    tiles:  a plane batch (``_plane_batch``), H and W at most 65535.
    shifts: one pair (Sy, Sx) of integers in 1/256 pixel, each in -16384..16384, for every plane, or a sequence of one pair per
            index of the leading dimension (all planes under that index take it).  (0, 0) gives an exact copy.
    out:    None, or the tensor to fill: ``_out_of_place``.
    Returns ``out``."""
    src = _plane_batch(tiles, 'tiles')
    n_images, h, w, src_plane_stride, src_pitch = src
    shift = (-SQ_SHIFT_MAX, SQ_SHIFT_MAX, 'channel shift (1/256 pixel)')
    host, n_pairs = _tuple_table(shifts, tiles, (shift, shift), 'shifts', 'a pair (Sy, Sx)')
    if h > SQ_SHIFT_MAX_SIDE or w > SQ_SHIFT_MAX_SIDE:
        raise ValueError(f"planes of {h} x {w} have a side above {SQ_SHIFT_MAX_SIDE}")
    with _on_stream(stream):
        out, (_, _, _, dst_plane_stride, dst_pitch) = _out_of_place(out, tuple(tiles.shape), tiles, src, 'shift', stream)
        if n_images == 0:
            return out
        _check(lib().sq_shift_tiles(tiles.data_ptr(), out.data_ptr(), n_images, h, w, src_plane_stride, src_pitch,
                                    dst_plane_stride, dst_pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)), host,
                                    n_images // n_pairs, _stream_ptr(stream)), 'sq_shift_tiles')
    return out


SQ_AFFINE_MAX_PPM = 50000
SQ_AFFINE_MAX_SIDE = 65535
SQ_AFFINE_PLANES_PER_THREAD = 16


def affine_tiles(tiles, params, out=None, stream=None):
    """Affine map about the plane's centre, composed with a constant shift, of every H x W plane of ``tiles`` into ``out``
    (sq_affine_tiles; an extension, the reference has nothing like it): the output at centre + p takes the input at centre +
    (1 + A 10^-6) p + S/256, bilinearly with 8 fractional bits and replicated edges, exact in integers --
    ``tests/affine_ref.affine_image``; the formula stands in include/squidstitch.h.  With A = 0 it is ``shift_tiles``.  The map is
    out of place: ``tiles`` is left as it is.

    tiles:  a plane batch (``_plane_batch``), H and W at most 65535.
    params: one six-tuple (Sy, Sx, Ayy, Ayx, Axy, Axx) of integers -- S in 1/256 pixel, each in -16384..16384, A in parts per
            million, each in -50000..50000 -- for every plane, or a sequence of one six-tuple per index of the leading dimension
            (all planes under that index take it).  All zero gives an exact copy.
    out:    None, or the tensor to fill: ``_out_of_place``.
    Returns ``out``."""
    src = _plane_batch(tiles, 'tiles')
    n_images, h, w, src_plane_stride, src_pitch = src
    shift = (-SQ_SHIFT_MAX, SQ_SHIFT_MAX, 'channel shift (1/256 pixel)')
    coeff = (-SQ_AFFINE_MAX_PPM, SQ_AFFINE_MAX_PPM, 'channel affine coefficient (ppm)')
    host, n_tuples = _tuple_table(params, tiles, (shift, shift, coeff, coeff, coeff, coeff), 'params',
                                  'a six-tuple (Sy, Sx, Ayy, Ayx, Axy, Axx)')
    if h > SQ_AFFINE_MAX_SIDE or w > SQ_AFFINE_MAX_SIDE:
        raise ValueError(f"planes of {h} x {w} have a side above {SQ_AFFINE_MAX_SIDE}")
    with _on_stream(stream):
        out, (_, _, _, dst_plane_stride, dst_pitch) = _out_of_place(out, tuple(tiles.shape), tiles, src, 'map', stream)
        if n_images == 0:
            return out
        _check(lib().sq_affine_tiles(tiles.data_ptr(), out.data_ptr(), n_images, h, w, src_plane_stride, src_pitch,
                                     dst_plane_stride, dst_pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)), host,
                                     n_images // n_tuples, _stream_ptr(stream)), 'sq_affine_tiles')
    return out


SQ_DARK_IMAGES_PER_THREAD = 1
DARK_DEFINITION = 'out = clamp(I - D + P, 0, M): D the dark frame (or a constant), P the pedestal, M = the dtype maximum'


def dark_tiles(tiles, params, frames=None, pedestal: int = 0, stream=None):
    """Dark-frame subtraction of every H x W plane of ``tiles``, IN PLACE (sq_dark_tiles; an extension, the reference has none):
    clamp(I - D + P, 0, M) with M the dtype's maximum, exact in integers -- ``tests/dark_ref.dark_image``; the formula stands in
    include/squidstitch.h.

    tiles:    a plane batch (``_plane_batch``).
    params:   one pair (k, c) of integers for every plane, or a sequence of one pair per index of the leading dimension (all
              planes under that index take it): k >= 0 names frame k of ``frames`` (with c == 0), k == -1 the constant c in 0..M.
              A run of pairs that is the identity (k == -1, c == pedestal) launches nothing.
    frames:   None, or a device tensor [K, H, W] / [H, W] of the tiles' dtype under the same layout rules that shares no memory
              with ``tiles``.
    pedestal: P, an integer in 0..M.
    Returns ``tiles``."""
    import torch
    lay = _plane_batch(tiles, 'tiles')
    n_images, h, w, plane_stride, pitch = lay
    top = 255 if tiles.dtype == torch.uint8 else 65535
    pedestal = _int_in(pedestal, 0, top, 'dark pedestal')
    n_frames = 0
    lay_f = None
    if frames is not None:
        if not torch.is_tensor(frames) or frames.dim() not in (2, 3) or frames.dtype != tiles.dtype or \
                frames.device != tiles.device or tuple(frames.shape[-2:]) != tuple(tiles.shape[-2:]):
            raise ValueError(f"frames must be a {tiles.dtype} tensor [K, {tiles.shape[-2]}, {tiles.shape[-1]}] on the tiles' device")
        lay_f = _plane_layout(frames, 'frames')
        n_frames = lay_f[0]
    host, n_pairs = _tuple_table(params, tiles, ((-1, n_frames - 1, 'dark frame index'), (0, top, 'dark constant')), 'params',
                                 'a pair (k, c)')
    for k, c in zip(host[0::2], host[1::2]):
        if k >= 0:
            _int_in(c, 0, 0, 'dark constant')      # a frame takes no constant
    if n_images == 0:
        return tiles
    if lay_f is not None and n_frames and _overlap(_byte_extent(tiles, lay), _byte_extent(frames, lay_f)):
        raise ValueError("frames shares memory with tiles")
    _check(lib().sq_dark_tiles(tiles.data_ptr(), n_images, h, w, plane_stride, pitch, sq_dtype_of(np_dtype_of_torch(tiles.dtype)),
                               frames.data_ptr() if n_frames else None, n_frames, lay_f[3] if n_frames else 0,
                               lay_f[4] if n_frames else 0, host, n_images // n_pairs, pedestal, _stream_ptr(stream)),
           'sq_dark_tiles')
    return tiles


_COPY_STREAMS = {}


def _copy_stream(device):
    """One stream per device for small result read-backs, so that they do not queue behind whatever the
    caller has enqueued on its own stream since (e.g. a 35 ms fusion launch)."""
    import torch
    key = (device.type, device.index)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=device)
    return _COPY_STREAMS[key]


class PendingRegistration:
    """Results of an enqueued sq_register_pairs; ``fetch()`` waits for THAT batch (not for later work on
    the caller's stream) and returns them."""

    def __init__(self, res_dev, keep, n, done=None):
        self._res, self._keep, self._n, self._done = res_dev, keep, n, done

    def fetch(self) -> np.ndarray:
        import torch
        if self._n == 0:
            return np.zeros(0, dtype=RESULT_DTYPE)
        if self._done is not None:
            side = _copy_stream(self._res.device)
            side.wait_event(self._done)
            self._res.record_stream(side)
            with torch.cuda.stream(side):
                host = self._res.cpu()
        else:
            host = self._res.cpu()
        out = host.numpy().view(RESULT_DTYPE).copy()
        self._keep = None
        return out


def _check_pairs(pairs, n_tiles: int, h: int, w: int, n0: int, n1: int) -> np.ndarray:
    """``pairs`` as contiguous PAIR_DTYPE records, every tile index in 0..n_tiles-1 and every n0 x n1 crop inside its h x w
    tile; ValueError otherwise.  The origins are int32 and may sit anywhere up to 2^31 - 1, where origin + side wraps in int32:
    they are compared in int64, with the room a crop has in its tile."""
    pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE).reshape(-1)
    if len(pairs) == 0:
        return pairs
    fields = pairs.view(np.int32).reshape(-1, 6).astype(np.int64)      # (ref_tile, mov_tile, ref_y0, ref_x0, mov_y0, mov_x0)
    if fields[:, :2].min() < 0 or fields[:, :2].max() >= n_tiles:
        raise ValueError("pair refers to a tile outside the table")
    room_y, room_x = int(h) - int(n0), int(w) - int(n1)                # Python integers: the last origin inside the tile
    if fields[:, 2:].min() < 0 or (fields[:, 2:] > np.array([room_y, room_x, room_y, room_x], dtype=np.int64)).any():
        raise ValueError("crop reaches outside its tile")
    return pairs


def register_pairs_async(tiles, minmax, pairs: np.ndarray, n0: int, n1: int, upsample_factor: int = 10,
                         normalization: int = SQ_NORM_PHASE, stream=None, tile_ptrs=None, shape=None,
                         np_dtype=None) -> PendingRegistration:
    """Enqueue batched phase cross-correlation of crop pairs and return without synchronising.
    ``tiles`` [N, H, W] device stack (or a pointer table + shape + dtype), ``pairs`` PAIR_DTYPE."""
    import torch
    ptrs, base, stride, n, h, w, dt, device = _tile_table(tiles, tile_ptrs, shape, np_dtype)
    pairs = _check_pairs(pairs, n, h, w, n0, n1)
    npairs = len(pairs)
    if npairs == 0:
        return PendingRegistration(None, None, 0)
    L = lib()
    ws_bytes = _size(L.sq_register_workspace_bytes(npairs, n0, n1, upsample_factor), 'sq_register_workspace_bytes')
    with _on_stream(stream):
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        pairs_dev = upload_small(torch.from_numpy(pairs.view(np.uint8).reshape(-1)), device)
        res_dev = torch.zeros(npairs * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=device)
        a = _RegisterArgs()
        a.tile_ptrs_dev = ptrs
        a.tile_base_dev = base
        a.tile_stride = stride
        a.n_tiles, a.tile_h, a.tile_w, a.tile_pitch = n, h, w, w
        a.tile_dtype = dt
        a.minmax_dev = minmax.data_ptr()
        a.pairs_dev = pairs_dev.data_ptr()
        a.n_pairs = npairs
        a.n0, a.n1 = int(n0), int(n1)
        a.upsample_factor = int(upsample_factor)
        a.normalization = int(normalization)
        a.results_dev = res_dev.data_ptr()
        a.workspace_dev = ws.data_ptr()
        a.workspace_bytes = ws.numel()
        _check(L.sq_register_pairs(C.byref(a), _stream_ptr(stream)), 'sq_register_pairs')
        done = torch.cuda.Event()
        done.record(stream if stream is not None else torch.cuda.current_stream())
    return PendingRegistration(res_dev, (ws, pairs_dev, minmax, tiles, tile_ptrs), npairs, done)


def register_pairs(tiles, minmax, pairs: np.ndarray, n0: int, n1: int, upsample_factor: int = 10,
                   normalization: int = SQ_NORM_PHASE, stream=None, tile_ptrs=None, shape=None,
                   np_dtype=None) -> np.ndarray:
    """register_pairs_async + fetch: returns a RESULT_DTYPE host array (synchronises)."""
    return register_pairs_async(tiles, minmax, pairs, n0, n1, upsample_factor, normalization, stream,
                                tile_ptrs, shape, np_dtype).fetch()


def register_describe(n_pairs: int, n0: int, n1: int, upsample_factor: int = 10, np_dtype='uint16') -> dict:
    """The launches sq_register_pairs issues for such a batch (sq_register_plan as a dict; host only, no device needed):
    ``radix0`` / ``radix1`` are the stage lists (empty for a power of two), ``upsample_rows`` is the (TB, KC) instantiation
    of the first upsampling kernel or None at ``upsample_factor`` 1, the grids are (x, y) tuples."""
    plan = _RegisterPlan()
    _check(lib().sq_register_describe(int(n_pairs), int(n0), int(n1), int(upsample_factor), sq_dtype_of(np_dtype), C.byref(plan)),
           'sq_register_describe')
    d = {name: getattr(plan, name) for name in (
        'm0', 'm1', 'tc', 'share', 'col_threads', 'columns_single_threads', 'rl_fwd', 'rl_inv', 'threads_fwd', 'threads_inv',
        'lds_fwd', 'lds_col', 'lds_inv')}
    for name in ('long0', 'long1', 'gen0', 'gen1', 'columns_single'):
        d[name] = bool(getattr(plan, name))
    d['radix0'] = [int(r) for r in plan.radix0[:plan.nf0]]
    d['radix1'] = [int(r) for r in plan.radix1[:plan.nf1]]
    d['upsample_rows'] = (plan.upsample_rows_tb, plan.upsample_rows_kc) if plan.upsample_rows_tb else None
    for name in ('grid_fwd', 'grid_col', 'grid_inv', 'grid_up_rows'):
        d[name] = tuple(int(v) for v in getattr(plan, name))
    return d


def write_files(paths: Sequence[str], data: np.ndarray, data_offsets: np.ndarray, n_threads: int = 16) -> int:
    """Write ``len(paths)`` files with native threads (sq_write_files): file i holds ``data[data_offsets[i]:data_offsets[i + 1]]``
    (``data`` a contiguous uint8 array, ``data_offsets`` int64 with one more entry than there are paths).  The directories must
    exist.  Returns the bytes written.  What the chunk writer of the OME-Zarr store uses: tens of thousands of half-MB files per
    batch, which Python's own open / write / close serialised under the interpreter lock."""
    n = len(paths)
    if n == 0:
        return 0
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    offs = np.ascontiguousarray(data_offsets, dtype=np.int64)
    if offs.shape != (n + 1,) or offs[0] < 0 or offs[-1] > data.size:
        raise ValueError("data_offsets needs len(paths) + 1 non-decreasing entries inside the data")
    encoded = [os.fsencode(p) + b'\0' for p in paths]
    poffs = np.zeros(n, dtype=np.int64)
    np.cumsum([len(e) for e in encoded[:-1]], out=poffs[1:])
    blob = b''.join(encoded)
    done = C.c_int64(0)
    _check(lib().sq_write_files(blob, poffs.ctypes.data, data.ctypes.data, offs.ctypes.data, n, int(n_threads), C.byref(done)),
           'sq_write_files')
    return int(done.value)


class _StreamBuffers:
    """Device buffers of one geometry of a packed-stream encoder (``sq_<codec>_encode_planes``): scratch, tile offsets, packed
    streams, status.  ``bound`` is the capacity of ``out``."""
    codec = ''

    def __init__(self, n_planes: int, h: int, w: int, dt: int, tile_h: int, tile_w: int, device, capacity: Optional[int] = None):
        import torch
        L = lib()
        self.geometry = (int(n_planes), int(h), int(w), dt, int(tile_h), int(tile_w))
        self.n_chunks = int(getattr(L, f'sq_{self.codec}_chunk_count')(n_planes, h, w, tile_h, tile_w))
        worst = int(getattr(L, f'sq_{self.codec}_out_bound')(*self.geometry))
        need = int(getattr(L, f'sq_{self.codec}_scratch_bytes')(*self.geometry))
        _size(min(self.n_chunks, worst, need), f'sq_{self.codec} geometry')
        self.bound = self._capacity(worst, capacity)
        self.scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
        self.offsets = torch.empty(self.n_chunks + 1, dtype=torch.int64, device=device)
        self.out = torch.empty(max(self.bound, 1), dtype=torch.uint8, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def _capacity(self, worst: int, capacity: Optional[int]) -> int:
        return worst

    def _out_capacity(self) -> int:      # what the entry point is told
        return self.out.numel()


class BloscBuffers(_StreamBuffers):
    """Device buffers of one sq_blosc_encode_planes geometry: scratch, chunk offsets, packed frames, status."""
    codec = 'blosc'

    def __init__(self, n_planes: int, h: int, w: int, np_dtype, chunk_h: int, chunk_w: int, device):
        super().__init__(n_planes, h, w, sq_dtype_of(np_dtype), chunk_h, chunk_w, device)


class DeflateBuffers(_StreamBuffers):
    """Device buffers of one sq_deflate_encode_planes geometry: scratch, tile offsets, packed zlib streams, status."""
    codec = 'deflate'

    def __init__(self, n_planes: int, h: int, w: int, np_dtype, tile_h: int, tile_w: int, device):
        super().__init__(n_planes, h, w, sq_dtype_of(np_dtype), tile_h, tile_w, device)


class JpegBuffers(_StreamBuffers):
    """Device buffers of one sq_jpeg_encode_planes geometry: scratch, tile offsets, packed JPEG streams, status.  ``bound`` is
    the capacity of ``out`` -- what a caller page-locks to fetch the streams: the tiles' raw bytes plus a header per tile, not
    sq_jpeg_out_bound()'s worst case (6.5 times raw, reached only by noise at the highest quality).  Tiles that do not fit set
    the status word and nothing is written; ``capacity`` overrides the default (``worst_case`` is the bound that never fails)."""
    codec = 'jpeg'

    def __init__(self, n_planes: int, h: int, w: int, tile_h: int, tile_w: int, device, capacity: Optional[int] = None):
        super().__init__(n_planes, h, w, SQ_U8, tile_h, tile_w, device, capacity)

    def _capacity(self, worst: int, capacity: Optional[int]) -> int:
        from . import jpegtile
        self.worst_case = worst
        if capacity is not None and int(capacity) < 0:
            raise ValueError(f"capacity must be >= 0, got {capacity}")
        th, tw = self.geometry[4:]
        return int(capacity) if capacity is not None else min(worst, self.n_chunks * (th * tw + jpegtile.HEADER_BYTES + 2))

    def _out_capacity(self) -> int:      # exactly ``bound``, also when it is 0
        return self.bound


def _encode_planes(codec: str, planes, nhw: tuple, dt: int, tile_h: int, tile_w: int, extra: tuple, buffers, make, stream,
                   capacity: Optional[int] = None):
    """The common part of the three ``*_encode_planes``, behind their own checks: the buffers of the geometry (``buffers`` when they
    are of it, else ``make()``), the strides and the call; ``extra`` are the codec's arguments behind the tile shape."""
    n, h, w = nhw
    with _on_stream(stream):
        if buffers is None or buffers.codec != codec or buffers.geometry != (n, h, w, dt, int(tile_h), int(tile_w)) \
                or (capacity is not None and buffers.bound != int(capacity)):
            buffers = make()
        fn = f'sq_{codec}_encode_planes'
        _check(getattr(lib(), fn)(planes.data_ptr(), planes.stride(0) if n > 1 else h * planes.stride(1), planes.stride(1), n, h, w, dt,
                                  int(tile_h), int(tile_w), *extra, buffers.scratch.data_ptr(), buffers.scratch.numel(),
                                  buffers.offsets.data_ptr(), buffers.out.data_ptr(), buffers._out_capacity(),
                                  buffers.status.data_ptr(), _stream_ptr(stream)), fn)
    return buffers


def blosc_encode_planes(planes, chunk_h: int, chunk_w: int, buffers: Optional[BloscBuffers] = None, stream=None) -> BloscBuffers:
    """Enqueue the Blosc-1 (shuffle + LZ4) encoding of the chunks of ``planes`` [n, H, W] (uint8 / uint16 device tensor,
    unit-stride rows, any pitch / plane stride).  Returns the buffers: after the stream has run, chunk i (plane-major,
    chunk row, chunk column) is ``buffers.out[offsets[i]:offsets[i + 1]]`` with ``offsets = buffers.offsets``
    (size 0 = all-zero chunk).  Nothing is synchronised or copied here."""
    n, h, w = _plane_stack(planes, 'planes', integer_only=False)
    npdt = np_dtype_of_torch(planes.dtype)
    return _encode_planes('blosc', planes, (n, h, w), sq_dtype_of(npdt), chunk_h, chunk_w, (), buffers,
                          lambda: BloscBuffers(n, h, w, npdt, chunk_h, chunk_w, planes.device), stream)


def deflate_encode_planes(planes, tile_h: int, tile_w: int, predictor: int = 2, buffers: Optional[DeflateBuffers] = None,
                          stream=None) -> DeflateBuffers:
    """Enqueue the zlib (RFC 1950) encoding of the TIFF tiles of ``planes`` [n, H, W] (uint8 / uint16 device tensor, unit-stride
    rows, any pitch / plane stride; tiles are full, zero past the plane's edge; ``predictor`` 2 = horizontal differencing, 1 =
    none).  Returns the buffers: after the stream has run, tile i (plane-major, tile row, tile column) is
    ``buffers.out[offsets[i]:offsets[i + 1]]`` with ``offsets = buffers.offsets`` (size 0 = all-zero tile).  Nothing is
    synchronised or copied here."""
    n, h, w = _plane_stack(planes, 'planes', integer_only=False)
    npdt = np_dtype_of_torch(planes.dtype)
    predictor = _int_in(predictor, 1, 2, 'predictor')
    return _encode_planes('deflate', planes, (n, h, w), sq_dtype_of(npdt), tile_h, tile_w, (predictor,), buffers,
                          lambda: DeflateBuffers(n, h, w, npdt, tile_h, tile_w, planes.device), stream)


def jpeg_overflow_message(quality: int) -> str:
    """What a caller reports when ``JpegBuffers.status`` came back non-zero with the default capacity."""
    return (f"sq_jpeg_encode_planes: the tiles of a batch did not shrink below their raw size at quality {quality} (noise, not an "
            f"image?); lower --ome-tiff-quality or write this data with --ome-tiff-compression deflate")


def jpeg_encode_planes(planes, tile_h: int, tile_w: int, quality: int = 90, buffers: Optional[JpegBuffers] = None,
                       stream=None, capacity: Optional[int] = None) -> JpegBuffers:
    """Enqueue the baseline JPEG encoding (TIFF Compression 7; include/squidstitch.h, stated in numpy by jpegtile.py) of the TIFF
    tiles of ``planes`` [n, H, W] (uint8 device tensor, unit-stride rows, any pitch / plane stride; tiles are full, zero past
    the plane's edge; sides multiples of 8).  Returns the buffers: after the stream has run, tile i (plane-major, tile row, tile
    column) is ``buffers.out[offsets[i]:offsets[i + 1]]`` (size 0 = all-zero tile) unless ``buffers.status`` is non-zero: then
    ``buffers.bound`` was too small and nothing was written.  Nothing is synchronised or copied here."""
    n, h, w = _plane_stack(planes, 'planes', integer_only=False)
    quality = _int_in(quality, 1, 100, 'quality')
    _size(lib().sq_jpeg_out_bound(n, h, w, sq_dtype_of(np_dtype_of_torch(planes.dtype)), int(tile_h), int(tile_w)),
          'sq_jpeg_encode_planes')      # (the entry point's refusal of anything but uint8, before buffers are made for it)
    return _encode_planes('jpeg', planes, (n, h, w), SQ_U8, tile_h, tile_w, (quality,), buffers,
                          lambda: JpegBuffers(n, h, w, tile_h, tile_w, planes.device, capacity=capacity), stream, capacity)


def basic_fit(tiles, smoothness_flatfield: float = 1.0, stream=None):
    """Flatfield estimate of a device stack [n, H, W] (uint8 / uint16, n <= 80) -> (device float32 [H, W], info dict).
    Replaces ``BaSiC(get_darkfield=False, smoothness_flatfield=...).fit(images).flatfield`` (stitcher.py:374-377);
    parity with basicpy is UNPINNED (the package is absent offline) -- see include/squidstitch.h.  Synchronises.
    ``info['capped_rounds']`` counts the re-weighting rounds that stopped at the 500-iteration cap (0 for a fit that
    settled); a fit whose 128 x 128 flatfield is not finite and > 0 everywhere raises NativeError with status
    SQ_ERR_NUMERIC instead of returning gains that would ruin the fusion divide."""
    import torch
    L = lib()
    if tiles.dim() != 3 or not tiles.is_cuda or not tiles.is_contiguous():
        raise ValueError("tiles must be a contiguous [n, H, W] device tensor")
    n, h, w = (int(v) for v in tiles.shape)
    need = _size(L.sq_basic_workspace_bytes(n, h, w), 'sq_basic_workspace_bytes')
    with _on_stream(stream):
        ws = torch.empty(need, dtype=torch.uint8, device=tiles.device)
        out = torch.empty((h, w), dtype=torch.float32, device=tiles.device)
        info = _BasicInfo()
        _check(L.sq_basic_fit(None, tiles.data_ptr(), h * w, n, h, w, w, sq_dtype_of(np_dtype_of_torch(tiles.dtype)),
                              float(smoothness_flatfield), out.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(info),
                              _stream_ptr(stream)), 'sq_basic_fit')
    return out, {'reweight_iterations': info.reweight_iterations, 'ladmap_iterations': info.ladmap_iterations,
                 'working_size': info.working_size, 'capped_rounds': info.capped_rounds}


def _selftest(name: str, device, *args) -> int:
    """The mismatch count of self-test ``name``(*args, count, stream), whose kernels add into a zeroed device counter."""
    import torch
    out = torch.zeros(1, dtype=torch.int64, device=device)
    _check(getattr(lib(), name)(*args, out.data_ptr(), _stream_ptr()), name)
    return int(out.item())


def selftest_flat_divide(exponent: int, n_binades: int, negative: bool, device) -> int:
    """Mismatches between the fast and the IEEE flatfield divide over whole binades of gains (tests)."""
    return _selftest('sq_selftest_flat_divide', device, int(exponent), int(n_binades), int(bool(negative)))


def selftest_flat_divide_f64(exponent: int, n_binades: int, negative: bool, seed: int, device) -> int:
    """Mismatches between the shortened and the IEEE float64 flatfield divide on random gains (tests)."""
    return _selftest('sq_selftest_flat_divide_f64', device, int(exponent), int(n_binades), int(bool(negative)),
                     int(seed) & (2 ** 64 - 1))


def selftest_normalise_divide(device) -> int:
    """Mismatches between the registration kernels' shortened normalisation quotient and the IEEE float64 division over
    every (numerator, range) pair of 16-bit integers (tests)."""
    return _selftest('sq_selftest_normalise_divide', device)


def selftest_blend_divide(exponent: int, n_binades: int, negative: bool, device) -> int:
    """Mismatches between the grouped feather blend's final division and the IEEE one over whole binades (tests)."""
    return _selftest('sq_selftest_blend_divide', device, int(exponent), int(n_binades), int(bool(negative)))


def synth_tiles(desc: np.ndarray, tile_h: int, tile_w: int, noise_amp: int, np_dtype, device, out=None, stream=None):
    """Generate tiles on the device from SYNTH_DTYPE descriptors -> [n, H, W] tensor."""
    import torch
    L = lib()
    desc = np.ascontiguousarray(desc, dtype=SYNTH_DTYPE)
    n = len(desc)
    with _on_stream(stream):
        if out is None:
            out = torch.empty((n, tile_h, tile_w), dtype=torch_dtype_of(np_dtype), device=device)
        d = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(device)
        for i0 in range(0, n, 32768):   # grid.z limit
            i1 = min(n, i0 + 32768)
            _check(L.sq_synth_tiles(d.data_ptr() + i0 * SYNTH_DTYPE.itemsize, i1 - i0, tile_h, tile_w, noise_amp,
                                    sq_dtype_of(np_dtype), out[i0:].data_ptr(), _stream_ptr(stream)), 'sq_synth_tiles')
    return out
