"""himg_amd -- MI355X-native HIMG encode/decode engine (Python plumbing).

The product is the C-ABI shared library (include/himg_hip.h) built from the
hand-written HIP kernels under himg_amd/csrc/.  This module is only the ctypes
binding that tests, bench.py and the multi-GPU driver use; PyTorch supplies
device memory, streams and torch.distributed, nothing else.

There is no CPU fallback: if the native library cannot be loaded or no GPU is
usable, the compute entry points raise.
"""
import ctypes as C
import os

import numpy as np

from .build import LIB, build_lib

HIMG_OK = 0
HIMG_ERR_ARG = -1
HIMG_ERR_HIP = -2
HIMG_ERR_UNSUPPORTED = -3
HIMG_ERR_FORMAT = -4
HIMG_ERR_CAPACITY = -5
HIMG_ERR_TARGET = -6

HIMG_DT_F32 = 0
HIMG_DT_F16 = 1
HIMG_DT_BF16 = 2

SYNTH = {"grad": 0, "gradn": 1, "rand": 2, "randtile": 3}

# himg_hip_debug_read selectors (include/himg_hip.h)
DBG = {
    "avg": 0, "lowres": 1, "lres_sym": 2, "fres_sym": 3, "lres_hist": 4, "fres_hist": 5,
    "lres_len": 6, "fres_len": 7, "lres_code": 8, "fres_code": 9, "fres_row_bytes": 10,
    "dec_stats": 11, "parse_stats": 12, "rowcount_stats": 13, "loop_counts": 14, "fres_tok_sym": 15, "tok_cnt": 16,
    "lane_start": 17, "lane_off": 18,
}
DBG_DECODER = 0x100

_lib = None


class HimgError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("himg_hip error %d %s" % (code, msg))
        self.code = code


def lib():
    """Load (building if necessary) the native library; fail loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB
    if not os.path.exists(path):
        path = build_lib()
    # PyTorch bundles its own HIP runtime (same SONAME as /opt/rocm's).  Whichever
    # copy is loaded first serves the whole process, and torch cannot enumerate
    # GPUs through a foreign copy -- so when torch is installed let it load first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i32, u32, u64, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t
    P = C.POINTER
    L.himg_hip_create.argtypes = [i32, P(vp)]
    L.himg_hip_destroy.argtypes = [vp]
    L.himg_hip_destroy.restype = None
    L.himg_hip_last_error.argtypes = [vp]
    L.himg_hip_last_error.restype = C.c_char_p
    L.himg_hip_max_packed_size.argtypes = [i32, i32, i32]
    L.himg_hip_max_packed_size.restype = sz
    L.himg_hip_tok_layout.argtypes = [i32, i32, i32, i32, i32, i32, P(i32)]
    L.himg_hip_encode.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, P(vp), P(sz)]
    L.himg_hip_decode.argtypes = [vp, vp, sz, P(vp), P(i32), P(i32), P(i32)]
    L.himg_hip_encode_to.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, P(sz)]
    L.himg_hip_decode_to.argtypes = [vp, vp, sz, vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_fetch_last.argtypes = [vp, vp, sz, P(sz)]
    L.himg_hip_peek.argtypes = [vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_set_option.argtypes = [vp, i32, i32]
    L.himg_hip_get_option.argtypes = [vp, i32, C.POINTER(C.c_int)]
    L.himg_hip_encode_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_decode_batch.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.himg_hip_free.argtypes = [vp]
    L.himg_hip_free.restype = None
    L.himg_hip_host_alloc.argtypes = [sz]
    L.himg_hip_host_alloc.restype = vp
    L.himg_hip_host_free.argtypes = [vp]
    L.himg_hip_host_free.restype = None
    L.himg_hip_encode_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp]
    L.himg_hip_decode_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_debug_row_records.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp]
    L.himg_hip_encode_device_q.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, sz, vp, vp, vp]
    L.himg_hip_windows_extent.argtypes = [vp, i32, i32, vp, i32, i32, P(sz)]
    L.himg_hip_encode_windows_device.argtypes = [vp, vp, vp, i32, i32, vp, i32, i32, vp, i32, vp, sz, vp, vp, vp]
    L.himg_hip_encode_window_to.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, P(sz)]
    L.himg_hip_encode_sizes_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp]
    L.himg_hip_budget_probes.argtypes = [i32, i32]
    L.himg_hip_encode_budget_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp, vp, vp, vp]
    L.himg_hip_encode_budget_to.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, sz, vp, sz, P(sz), P(i32)]
    L.himg_hip_encode_budget_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.himg_hip_encode_sse_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, vp]
    L.himg_hip_encode_target_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp, vp, vp, vp, vp]
    L.himg_hip_encode_target_to.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, u64, vp, sz, P(sz), P(i32), P(u64)]
    L.himg_hip_encode_target_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.himg_hip_psnr_to_sse.argtypes = [C.c_double, i32, i32, i32, P(u64)]
    L.himg_hip_decode_rows_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_decode_index_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, vp, vp, vp, vp]
    L.himg_hip_decode_rows_indexed_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.himg_hip_decode_rows_after_head_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.himg_hip_decode_head_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, vp]
    L.himg_hip_decode_first_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_decode_walk_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, vp, vp, vp, vp]
    L.himg_hip_decode_walk_wait.argtypes = [vp]
    L.himg_hip_decode_walk_ranges_device.argtypes = [vp, vp, C.c_uint32, i32, i32, i32, C.POINTER(C.c_int), i32, vp, vp, vp, vp]
    L.himg_hip_decode_walk_wait_range.argtypes = [vp, i32]
    L.himg_hip_index_host.argtypes = [vp, sz, i32, P(i32), P(i32), P(i32), vp, sz, P(C.c_uint32)]
    L.himg_hip_preview_peek.argtypes = [vp, sz, sz, P(i32), P(i32), P(i32), P(sz)]
    L.himg_hip_region_peek.argtypes = [vp, sz, i32, i32, i32, i32, i32, vp]
    L.himg_hip_decode_region_to.argtypes = [vp, vp, sz, i32, i32, i32, i32, vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_decode_region_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_decode_regions_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp]
    L.himg_hip_decode_stream_regions_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp]
    L.himg_hip_stream_regions_peek.argtypes = [vp, sz, i32, i32, vp, i32, i32, vp, vp, P(i32)]
    L.himg_hip_decode_stream_regions_to.argtypes = [vp, vp, sz, i32, vp, i32, i32, vp, sz, vp, P(i32), P(i32), P(i32)]
    L.himg_hip_opened_bytes.argtypes = [i32, i32, i32, i32, P(sz)]
    L.himg_hip_open_streams_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, P(vp), vp]
    L.himg_hip_open_stream_host.argtypes = [vp, vp, sz, P(vp)]
    L.himg_hip_opened_regions_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.himg_hip_opened_regions_to.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, sz, vp, P(i32), P(i32), P(i32)]
    L.himg_hip_opened_scaled_regions_device.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]
    L.himg_hip_opened_scaled_regions_to.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, sz, vp, P(i32), P(i32), P(i32)]
    L.himg_hip_opened_info.argtypes = [vp, P(i32), P(i32), P(i32), P(i32), P(sz), P(C.c_longlong)]
    L.himg_hip_close_streams.argtypes = [vp, vp]
    L.himg_hip_close_streams.restype = None
    L.himg_hip_tensor_bytes.argtypes = [vp, i32, i32, i32, P(sz)]
    L.himg_hip_decode_tensor_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.himg_hip_decode_regions_tensor_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    L.himg_hip_planes_bytes.argtypes = [i32, C.c_uint32, i32, i32, P(sz)]
    L.himg_hip_peek_format.argtypes = [vp, sz, P(i32), P(i32), P(i32), P(i32)]
    L.himg_hip_decode_planes_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, C.c_uint32, vp, vp, vp]
    L.himg_hip_decode_planes_to.argtypes = [vp, vp, sz, C.c_uint32, vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_dst_extent.argtypes = [vp, i32, i32, vp, i32, i32, P(sz)]
    L.himg_hip_decode_into_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.himg_hip_decode_regions_into_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    L.himg_hip_decode_into_to.argtypes = [vp, vp, sz, vp, vp, i32, i32, P(i32), P(i32), P(i32)]
    L.himg_hip_decode_regions_batch.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.himg_hip_scaled_size.argtypes = [i32, i32, i32, P(i32), P(i32)]
    L.himg_hip_decode_scaled_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_decode_scaled_to.argtypes = [vp, vp, sz, i32, vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_decode_scaled_batch.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.himg_hip_pyramid_size.argtypes = [i32, i32, i32, P(i32), P(i32)]
    L.himg_hip_decode_pyramid_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_decode_pyramid_to.argtypes = [vp, vp, sz, vp, vp, P(i32), P(i32), P(i32)]
    L.himg_hip_scaled_region_peek.argtypes = [vp, sz, i32, i32, i32, i32, i32, i32, vp]
    L.himg_hip_decode_scaled_region_to.argtypes = [vp, vp, sz, i32, i32, i32, i32, i32, vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_decode_scaled_regions_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp]
    L.himg_hip_decode_scaled_regions_batch.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.himg_hip_preview_to.argtypes = [vp, vp, sz, vp, sz, P(i32), P(i32), P(i32)]
    L.himg_hip_preview_batch.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.himg_hip_preview_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_prefix_peek.argtypes = [vp, sz, i32, vp]
    L.himg_hip_decode_prefix_to.argtypes = [vp, vp, sz, vp, sz, P(i32), P(i32), P(i32), P(i32)]
    L.himg_hip_decode_prefix_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.himg_hip_prefix_peek_from.argtypes = [vp, sz, i32, vp, vp]
    L.himg_hip_decode_prefix_more_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.himg_hip_decode_prefix_more_to.argtypes = [vp, vp, sz, vp, vp, sz, P(i32), P(i32), P(i32), P(i32)]
    L.himg_hip_decode_conceal_to.argtypes = [vp, vp, sz, vp, sz, P(i32), P(i32), P(i32), vp, sz, P(i32)]
    L.himg_hip_decode_conceal_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.himg_hip_create_multi.argtypes = [vp, i32, P(vp)]
    L.himg_hip_destroy_multi.argtypes = [vp]
    L.himg_hip_destroy_multi.restype = None
    L.himg_hip_multi_count.argtypes = [vp]
    L.himg_hip_multi_last_error.argtypes = [vp]
    L.himg_hip_multi_last_error.restype = C.c_char_p
    L.himg_hip_multi_set_option.argtypes = [vp, i32, i32]
    L.himg_hip_multi_encode_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_multi_decode_batch.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.himg_hip_multi_encode.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, P(vp), P(sz)]
    L.himg_hip_multi_decode.argtypes = [vp, vp, sz, P(vp), P(i32), P(i32), P(i32)]
    L.himg_hip_shard_stats.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.himg_hip_shard_row_bits.argtypes = [vp, vp, vp, vp]
    L.himg_hip_shard_emit.argtypes = [vp, vp, vp, sz, vp, vp]
    L.himg_hip_shard_assemble.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, vp, vp]
    L.himg_hip_shard_head.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp]
    L.himg_hip_shard_finish.argtypes = [vp, vp, sz, vp, vp]
    L.himg_hip_debug_read.argtypes = [vp, i32, i32, vp, sz, P(sz)]
    L.himg_hip_debug_trees.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.himg_hip_profile_enable.argtypes = [vp, i32]
    L.himg_hip_profile_reset.argtypes = [vp]
    L.himg_hip_profile_read.argtypes = [vp, P(i32), P(C.c_char_p), P(C.c_double), P(i32)]
    L.himg_synth_fill.argtypes = [i32, u64, i32, i32, vp]
    L.himg_fnv1a64.argtypes = [vp, sz]
    L.himg_fnv1a64.restype = u64
    L.himg_tables_shift.argtypes = [i32, i32, vp]
    L.himg_tables_shift.restype = None
    L.himg_tables_lowres_map.argtypes = [i32, vp]
    L.himg_tables_lowres_map.restype = None
    L.himg_tables_fullres_map.argtypes = [vp]
    L.himg_tables_fullres_map.restype = None
    L.himg_tables_map_to_8bit.argtypes = [vp, i32]
    L.himg_tables_map_to_8bit.restype = C.c_uint8
    _lib = L
    return L


# ---- host utilities (no GPU) -------------------------------------------------

def synth(kind, seed, width, height):
    """Synthetic RGBA frame as a (H, W, 4) uint8 array."""
    a = np.empty((height, width, 4), np.uint8)
    rc = lib().himg_synth_fill(SYNTH[kind], seed, width, height, a.ctypes.data)
    if rc:
        raise HimgError(rc, "synth")
    return a


def fnv1a64(buf):
    b = np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else buf)
    return "%016x" % lib().himg_fnv1a64(b.ctypes.data, b.nbytes)


def max_packed_size(width, height, channels):
    return int(lib().himg_hip_max_packed_size(width, height, channels))


def budget_probes(qmin=0, qmax=100):
    """himg_hip_budget_probes (no GPU): the size probes an encode to a byte budget makes for the
    quality range [qmin, qmax].  Raises HimgError (HIMG_ERR_ARG) unless 0 <= qmin <= qmax <= 100."""
    n = lib().himg_hip_budget_probes(int(qmin), int(qmax))
    if n < 0:
        raise HimgError(n, "budget_probes")
    return n


def psnr_to_sse(psnr_db, width, height, channels):
    """himg_hip_psnr_to_sse (no GPU): the largest sum of squared differences with which a width x
    height x channels picture still has at least psnr_db dB (the target of Engine.encode_target).
    Raises HimgError (HIMG_ERR_ARG) for a non-finite or negative dB or a bad geometry."""
    v = C.c_uint64()
    rc = lib().himg_hip_psnr_to_sse(float(psnr_db), int(width), int(height), int(channels), C.byref(v))
    if rc:
        raise HimgError(rc, "psnr_to_sse")
    return v.value


def tok_layout(width, height, channels=4, pixel_stride=None, row_tokens=-1, batch=1):
    """The encoder's token-stream layout for a geometry (himg_hip_tok_layout; no GPU needed): symbols per
    segment, segments per block row, slots a segment owns, the slots half an iteration of k_tok can
    stage and the slots its stage holds, and whether such an encode takes the token stream."""
    out = (C.c_int32 * 6)()
    rc = lib().himg_hip_tok_layout(width, height, pixel_stride or channels, channels, row_tokens, batch, out)
    if rc != 0:
        raise ValueError("himg_hip_tok_layout: %d" % rc)
    return {"seg": out[0], "nseg": out[1], "cap": out[2], "stage_need": out[3], "stage": out[4], "tokens": bool(out[5])}


def pinned_empty(nbytes):
    """uint8 numpy array in page-locked host memory (himg_hip_host_alloc): the host
    API's transfers from / to it are asynchronous DMA.  The allocation is released when
    the ctypes buffer behind the array -- which every view of it keeps alive -- is
    collected."""
    import weakref
    ptr = lib().himg_hip_host_alloc(int(nbytes))
    if not ptr:
        raise MemoryError("himg_hip_host_alloc(%d)" % nbytes)
    buf = (C.c_uint8 * int(nbytes)).from_address(ptr)
    weakref.finalize(buf, lib().himg_hip_host_free, ptr)
    return np.frombuffer(buf, np.uint8)


def psnr(a, b):
    """PSNR over all channels, 10*log10(255^2/MSE), double precision."""
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float(np.mean(d * d))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


# ---- engine ------------------------------------------------------------------

# himg_hip_get_option / himg_hip_set_option: the options by name (HIMG_OPT_*, include/himg_hip.h).
_OPTIONS = {"fix_t2": 1, "count_wave": 2, "emit_rows": 3, "row_tokens": 4, "front": 5, "count_stretch": 6}


class Engine:
    """One C-ABI context (one device).  Mirrors the reference's Encoder/Decoder
    pair: encode()/decode() take and return host buffers like
    himg::Encoder::Encode / himg::Decoder::Decode; the *_device methods work on
    HBM-resident batches (torch CUDA tensors or raw device pointers)."""

    def __init__(self, device=0):
        self._ctx = C.c_void_p()
        rc = lib().himg_hip_create(device, C.byref(self._ctx))
        if rc:
            raise HimgError(rc, "himg_hip_create (no usable GPU? there is no CPU fallback)")
        self.device = device
        # What the context took from the environment (HIMG_FIX_T2=1) counts too: the row-sharded
        # decoder's host index must follow the engine's own rule (sharded.py).
        self.fix_t2 = bool(self.get_option("fix_t2"))

    def close(self):
        if self._ctx:
            lib().himg_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise HimgError(rc, "%s: %s" % (what, lib().himg_hip_last_error(self._ctx).decode()))

    def _batch(self, fn, what, streams, outs, frame_bytes, *mid):
        """What the batch decodes share: streams and output buffers into ctypes arrays, the call
        fn(ctx, streams, sizes, n, *mid, outs, capacities, widths, heights, channels), the results as
        (h, w, c) views of the buffers.  frame_bytes(i, stream): the size of a missing buffer (0 for a
        stream that cannot be sized: its frame fails in the call)."""
        n = len(streams)
        if outs is None:
            outs = [np.empty(max(frame_bytes(i, s_) or 0, 1), np.uint8) for i, s_ in enumerate(streams)]
        src = (C.c_void_p * n)(*[s_.ctypes.data for s_ in streams])
        szs = (C.c_size_t * n)(*[s_.nbytes for s_ in streams])
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
        ws, hs, cs = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        self._check(fn(self._ctx, src, szs, n, *mid, dst, caps, ws, hs, cs), what)
        return [o.ravel()[: ws[i] * hs[i] * cs[i]].reshape(hs[i], ws[i], cs[i]) for i, o in enumerate(outs)]

    def _encode_to(self, fn, what, img, channels, pixel_stride, mid, **results):
        """What the single-frame encodes share: fn(ctx, pixels, w, h, stride, ch, *mid, None, 0, &size,
        *&results) -- the call without a buffer, which reports the size with HIMG_ERR_CAPACITY -- then
        himg_hip_fetch_last into an array of exactly that size (no intermediate copies).  Returns
        (stream, *results); any other outcome raises HimgError with the results as attributes."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w, ch, stride = _image_geom(img, channels, pixel_stride)
        n = C.c_size_t()
        rc = fn(self._ctx, img.ctypes.data, w, h, stride, ch, *mid, None, 0, C.byref(n),
                *[C.byref(v) for v in results.values()])
        if rc != HIMG_ERR_CAPACITY or n.value == 0:
            e = HimgError(rc if rc != HIMG_OK else HIMG_ERR_ARG,
                          "%s: %s" % (what, lib().himg_hip_last_error(self._ctx).decode()))
            for name, v in results.items():
                setattr(e, name, v.value)
            raise e
        out = np.empty(n.value, np.uint8)
        self._check(lib().himg_hip_fetch_last(self._ctx, out.ctypes.data, out.nbytes, C.byref(n)), what)
        return (out, *[v.value for v in results.values()])

    def _encode_batch(self, fn, what, frames, outs, mid, results=(), soft=()):
        """What the batch encodes share: frames of one geometry and output buffers (`outs`: reusable
        uint8 buffers of at least max_packed_size bytes, else new ones) into ctypes arrays, the call
        fn(ctx, frames, n, w, h, stride, ch, *mid, outs, capacities, sizes, *results).  Returns (the
        streams as views into the buffers, rc): rc other than HIMG_OK or one of `soft` raises."""
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        n = len(frames)
        h, w, ch, stride = _image_geom(frames[0])
        if outs is None:
            outs = [np.empty(max_packed_size(w, h, ch), np.uint8) for _ in range(n)]
        src = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
        sizes = (C.c_size_t * n)()
        rc = fn(self._ctx, src, n, w, h, stride, ch, *mid, dst, caps, sizes, *results)
        if rc not in (HIMG_OK, *soft):
            self._check(rc, what)
        return [o[: sizes[i]] for i, o in enumerate(outs)], rc

    # host-buffer API ---------------------------------------------------------
    def encode(self, img, quality=50, use_ycbcr=True, channels=None, pixel_stride=None):
        """himg_hip_encode_to + himg_hip_fetch_last: the stream is fetched into an
        array of exactly its size (no intermediate copies)."""
        return self._encode_to(lib().himg_hip_encode_to, "encode", img, channels, pixel_stride,
                               (quality, 1 if use_ycbcr else 0))[0]

    def encode_window(self, data, src, x, y, w, h, quality=50, use_ycbcr=True, channels=None):
        """himg_hip_encode_window_to + himg_hip_fetch_last: the stream of the window (x, y, w, h) of the
        host picture `data` (uint8, laid out as `src` says: src_desc; channels: pixel_stride where not
        given).  Only the rows the window lies in are uploaded."""
        data = _as_u8(data)
        ch = src.pixel_stride if channels is None else channels
        n = C.c_size_t()
        rc = lib().himg_hip_encode_window_to(self._ctx, data.ctypes.data, C.byref(src), ch, int(x), int(y), int(w),
                                             int(h), quality, 1 if use_ycbcr else 0, None, 0, C.byref(n))
        if rc != HIMG_ERR_CAPACITY or n.value == 0:
            self._check(rc if rc != HIMG_OK else HIMG_ERR_ARG, "encode_window")
        out = np.empty(n.value, np.uint8)
        self._check(lib().himg_hip_fetch_last(self._ctx, out.ctypes.data, out.nbytes, C.byref(n)), "encode_window")
        return out

    def decode(self, packed, out=None):
        """himg_hip_peek + himg_hip_decode_to straight into `out` (reused when it has
        the right size) or a new array."""
        packed = np.ascontiguousarray(np.frombuffer(packed, np.uint8) if isinstance(packed, (bytes, bytearray)) else packed)
        w, h, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        geom = _peek(packed)
        if geom:
            out = _out_buffer(out, geom[0] * geom[1] * geom[2])
            dst, cap = out.ctypes.data, out.nbytes
        rc = lib().himg_hip_decode_to(self._ctx, packed.ctypes.data, packed.nbytes, dst, cap,
                                      C.byref(w), C.byref(h), C.byref(c))
        self._check(rc, "decode")
        return out.reshape(h.value, w.value, c.value)

    def encode_batch(self, frames, quality=50, use_ycbcr=True, outs=None):
        """himg_hip_encode_batch: frames of one geometry, transfers overlapped with the
        kernels.  `outs` (optional) are reusable uint8 buffers of at least
        max_packed_size bytes; returns the streams (views into outs when given)."""
        return self._encode_batch(lib().himg_hip_encode_batch, "encode_batch", frames, outs,
                                  (quality, 1 if use_ycbcr else 0))[0]

    def encode_budget(self, img, budget, qmin=0, qmax=100, use_ycbcr=True, channels=None, pixel_stride=None):
        """himg_hip_encode_budget_to + himg_hip_fetch_last: (stream, quality) -- the stream of at most
        `budget` bytes at the quality the search of include/himg_hip.h finds in [qmin, qmax].  Raises
        HimgError (HIMG_ERR_CAPACITY, its `quality` -1) when the stream at qmin is larger than the budget."""
        return self._encode_to(lib().himg_hip_encode_budget_to, "encode_budget", img, channels, pixel_stride,
                               (int(qmin), int(qmax), 1 if use_ycbcr else 0, max(int(budget), 0)), quality=C.c_int(-1))

    def encode_budget_batch(self, frames, budgets, qmin=0, qmax=100, use_ycbcr=True, outs=None):
        """himg_hip_encode_budget_batch: frames of one geometry, frame i within budgets[i] bytes.
        Returns (streams, qualities, rc): a frame whose budget is below its size at qmin (or that
        failed otherwise) has an empty stream and, for the budget, quality -1; rc is the first such
        error, HIMG_OK if there was none."""
        n = len(frames)
        bud = (C.c_size_t * n)(*[max(int(b), 0) for b in budgets])
        quals = (C.c_int * n)()
        streams, rc = self._encode_batch(lib().himg_hip_encode_budget_batch, "encode_budget_batch", frames, outs,
                                         (int(qmin), int(qmax), 1 if use_ycbcr else 0, bud), (quals,),
                                         soft=(HIMG_ERR_CAPACITY,))
        return streams, list(quals), rc

    def encode_target(self, img, max_sse, qmin=0, qmax=100, use_ycbcr=True, channels=None, pixel_stride=None):
        """himg_hip_encode_target_to + himg_hip_fetch_last: (stream, quality, sse) -- the stream at the
        quality the search of include/himg_hip.h finds in [qmin, qmax] for a sum of squared differences
        of at most `max_sse` (psnr_to_sse turns a PSNR into one), and the sum it has.  Raises HimgError
        (HIMG_ERR_TARGET, its `quality` -1 and its `sse` the sum at qmax) when qmax misses the target."""
        return self._encode_to(lib().himg_hip_encode_target_to, "encode_target", img, channels, pixel_stride,
                               (int(qmin), int(qmax), 1 if use_ycbcr else 0, min(max(int(max_sse), 0), 2 ** 64 - 1)),
                               quality=C.c_int(-1), sse=C.c_uint64())

    def encode_target_batch(self, frames, max_sses, qmin=0, qmax=100, use_ycbcr=True, outs=None):
        """himg_hip_encode_target_batch: frames of one geometry, frame i with a sum of squared
        differences of at most max_sses[i].  Returns (streams, qualities, sses, rc): a frame that
        misses its target at qmax (or that failed otherwise) has an empty stream and quality -1; rc is
        the first such error, HIMG_OK if there was none."""
        n = len(frames)
        tgt = (C.c_uint64 * n)(*[min(max(int(t), 0), 2 ** 64 - 1) for t in max_sses])
        quals, sses = (C.c_int * n)(), (C.c_uint64 * n)()
        streams, rc = self._encode_batch(lib().himg_hip_encode_target_batch, "encode_target_batch", frames, outs,
                                         (int(qmin), int(qmax), 1 if use_ycbcr else 0, tgt), (quals, sses),
                                         soft=(HIMG_ERR_TARGET,))
        return streams, list(quals), list(sses), rc

    def decode_batch(self, streams, outs=None):
        """himg_hip_decode_batch: returns the decoded frames; `outs` (optional) are
        reusable uint8 buffers large enough for the pixels."""
        streams = [np.ascontiguousarray(np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else s)
                   for s in streams]

        def frame_bytes(i, s_):
            geom = _peek(s_)
            return geom and geom[0] * geom[1] * geom[2]
        return self._batch(lib().himg_hip_decode_batch, "decode_batch", streams, outs, frame_bytes)

    def preview(self, packed, out=None, packed_size=None):
        """1/8-scale preview (himg_hip_preview_to): the low-res picture at the front of the
        stream as a (ceil(H/8), ceil(W/8), C) uint8 array.  `packed` may hold only the head of
        the stream (preview_peek's head_bytes); packed_size is then the whole stream's size."""
        packed = _as_u8(packed)
        size = packed.nbytes if packed_size is None else int(packed_size)
        pw, ph, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        hb = C.c_size_t()
        rc = lib().himg_hip_preview_peek(packed.ctypes.data, packed.nbytes, size, C.byref(pw), C.byref(ph), C.byref(c),
                                         C.byref(hb))
        if rc == HIMG_OK:
            out = _out_buffer(out, pw.value * ph.value * c.value)
            dst, cap = out.ctypes.data, out.nbytes
        elif rc != HIMG_ERR_FORMAT:
            # himg_hip_preview_to reads head_bytes from `packed` (its precondition): an array that
            # ends before the head (HIMG_ERR_CAPACITY) never reaches it.  (HIMG_ERR_FORMAT: the same
            # walk stops at the same place inside the array, and preview_to words the stage.)
            e = HimgError(rc, "preview: %s" % ("the array ends before the end of the LRES chunk (%d bytes)" % hb.value
                                               if rc == HIMG_ERR_CAPACITY else "unsupported stream"))
            e.head_bytes = hb.value
            raise e
        rc = lib().himg_hip_preview_to(self._ctx, packed.ctypes.data, size, dst, cap,
                                       C.byref(pw), C.byref(ph), C.byref(c))
        self._check(rc, "preview")
        return out.reshape(ph.value, pw.value, c.value)

    def preview_batch(self, streams, outs=None):
        """himg_hip_preview_batch: the previews of several streams (frames of one geometry
        share device launches of up to 256 frames); `outs` (optional) are reusable uint8 buffers."""
        def frame_bytes(i, s_):
            try:
                pw, ph, c, _ = preview_peek(s_)
                return pw * ph * c
            except HimgError:
                return 0
        return self._batch(lib().himg_hip_preview_batch, "preview_batch", [_as_u8(s_) for s_ in streams], outs,
                           frame_bytes)

    def preview_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, d_out,
                       d_status, stream=0):
        """himg_hip_preview_device: the contract of decode_device; d_out holds
        batch x ceil(H/8) x ceil(W/8) x C bytes."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_preview_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data,
                                           batch, width, height, channels, _ptr(d_out),
                                           _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "preview_device")

    def decode_prefix(self, prefix, out=None):
        """himg_hip_decode_prefix_to: `prefix` holds the first bytes of a stream, as many as have
        arrived.  Returns (picture, rows_complete): the (H, W, C) uint8 picture whose first
        rows_complete block rows are decode()'s and whose other rows come from the low-res plane alone
        (rows_complete = 0: all of it).  Raises HimgError -- HIMG_ERR_CAPACITY for a prefix that ends
        before the first row header (prefix_peek tells how many bytes that takes)."""
        prefix = _as_u8(prefix)
        w, h, c, k = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        plan = PrefixPlan()
        lib().himg_hip_prefix_peek(prefix.ctypes.data, prefix.nbytes, 0, C.byref(plan))
        if plan.num_channels:   # (the geometry is set as soon as FRMT is there and within the engine's limits)
            cap = plan.width * plan.height * plan.num_channels
            out = _out_buffer(out, cap)
            dst = out.ctypes.data
        rc = lib().himg_hip_decode_prefix_to(self._ctx, prefix.ctypes.data, prefix.nbytes, dst, cap, C.byref(w),
                                             C.byref(h), C.byref(c), C.byref(k))
        self._check(rc, "decode_prefix")
        return out.ravel()[: h.value * w.value * c.value].reshape(h.value, w.value, c.value), k.value

    def decode_prefix_device(self, d_packed, in_stride, h_avail, batch, width, height, channels, d_out, d_rows,
                             d_status, stream=0):
        """himg_hip_decode_prefix_device: the contract of decode_device with h_avail, the bytes present
        of each frame, where h_sizes stands; d_rows (batch x int32) receives each frame's complete
        block rows, -1 with a verdict."""
        ha = np.ascontiguousarray(h_avail, np.uint32)
        rc = lib().himg_hip_decode_prefix_device(self._ctx, _ptr(d_packed), in_stride, ha.ctypes.data, batch, width,
                                                 height, channels, _ptr(d_out), _ptr(d_rows), _ptr(d_status),
                                                 C.c_void_p(stream))
        self._check(rc, "decode_prefix_device")

    def decode_prefix_more(self, prefix, state, out=None):
        """himg_hip_decode_prefix_more_to: decode_prefix continued.  `state`: one element of
        prefix_states() (or a PrefixState), zeroed for the first call and kept with `out`, the (H, W, C)
        picture of the calls before; both are updated in place.  Only the block rows that became whole
        since the state's last call are decoded, uploaded for and copied back.  Returns (picture,
        rows_complete).  A first call may leave `out` None: the picture it returns is the one to pass on.
        Raises HimgError, the state unchanged."""
        prefix = _as_u8(prefix)
        st = state if isinstance(state, PrefixState) else PrefixState.from_buffer(_state_view(state))
        w, h, c, k = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        plan = PrefixPlan()
        lib().himg_hip_prefix_peek(prefix.ctypes.data, prefix.nbytes, 0, C.byref(plan))
        if plan.num_channels:
            cap = plan.width * plan.height * plan.num_channels
            if st.started and (out is None or out.nbytes != cap or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"]):
                raise ValueError("decode_prefix_more: a started state needs its picture, %d contiguous bytes" % cap)
            out = _out_buffer(out, cap)
            dst = out.ctypes.data
        rc = lib().himg_hip_decode_prefix_more_to(self._ctx, prefix.ctypes.data, prefix.nbytes, C.addressof(st), dst, cap,
                                                  C.byref(w), C.byref(h), C.byref(c), C.byref(k))
        self._check(rc, "decode_prefix_more")
        return out.ravel()[: h.value * w.value * c.value].reshape(h.value, w.value, c.value), k.value

    def decode_prefix_more_device(self, d_packed, in_stride, h_avail, batch, width, height, channels, d_state, d_out,
                                  d_rows, d_status, stream=0):
        """himg_hip_decode_prefix_more_device: decode_prefix_device continued from d_state -- batch
        16-byte states in device memory (prefix_states(batch) uploaded), read and advanced on the
        device: only the block rows that became whole since a frame's last call are decoded and written."""
        ha = np.ascontiguousarray(h_avail, np.uint32)
        rc = lib().himg_hip_decode_prefix_more_device(self._ctx, _ptr(d_packed), in_stride, ha.ctypes.data, batch, width,
                                                      height, channels, _ptr(d_state), _ptr(d_out), _ptr(d_rows),
                                                      _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_prefix_more_device")

    def decode_conceal(self, packed, out=None):
        """himg_hip_decode_conceal_to: the decode of a stream that may be damaged.  Returns (picture,
        rowmap): the (H, W, C) uint8 picture and a bool array with one entry per block row, True where
        the row was rejected or could not be delimited and was written from the low-res plane; every
        other row is decode()'s.  Raises HimgError, as decode() does, only for damage in the stream's
        head.  (No checksums: damage the decoder accepts is decoded as it stands.)"""
        packed = _as_u8(packed)
        w, h, c, n = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        dst, cap, rmap, rcap = None, 0, None, 0
        geom = _peek(packed)
        if geom:
            out = _out_buffer(out, geom[0] * geom[1] * geom[2])
            dst, cap = out.ctypes.data, out.nbytes
            rmap = np.zeros((geom[1] + 7) // 8, np.uint8)
            rcap = rmap.nbytes
        rc = lib().himg_hip_decode_conceal_to(self._ctx, packed.ctypes.data, packed.nbytes, dst, cap, C.byref(w),
                                              C.byref(h), C.byref(c), rmap.ctypes.data if geom else None, rcap,
                                              C.byref(n))
        self._check(rc, "decode_conceal")
        return out.reshape(h.value, w.value, c.value), rmap.astype(bool)

    def decode_conceal_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, d_out,
                              d_concealed, d_rowmap, d_status, stream=0):
        """himg_hip_decode_conceal_device: the contract of decode_device; d_concealed (batch x int32)
        receives each frame's concealed block rows, -1 with a head verdict; d_rowmap (batch x rows bytes,
        or None) the rows' map."""
        hs = None if h_sizes is None else np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_conceal_device(self._ctx, _ptr(d_packed), in_stride,
                                                  hs.ctypes.data if hs is not None else None, batch, width, height,
                                                  channels, _ptr(d_out), _ptr(d_concealed), _ptr(d_rowmap),
                                                  _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_conceal_device")

    def decode_region(self, packed, x, y, w, h, out=None):
        """Rectangle (x, y, w, h) at full resolution (himg_hip_decode_region_to) as an (h, w, C)
        uint8 array: pixel (i, j) is pixel (y + i, x + j) of decode().  Only the stream's head and
        the block rows the rectangle touches are uploaded (region_peek)."""
        packed = _as_u8(packed)
        wo, ho, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        geom = _peek(packed)
        if geom:
            cap = max(int(w), 0) * max(int(h), 0) * geom[2]
            out = _out_buffer(out, cap)
            dst = out.ctypes.data
        rc = lib().himg_hip_decode_region_to(self._ctx, packed.ctypes.data, packed.nbytes, int(x), int(y), int(w), int(h),
                                             dst, cap, C.byref(wo), C.byref(ho), C.byref(c))
        self._check(rc, "decode_region")
        return out.ravel()[: ho.value * wo.value * c.value].reshape(ho.value, wo.value, c.value)

    def decode_region_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, x, y, w, h,
                             d_out, d_status, stream=0):
        """himg_hip_decode_region_device: the contract of decode_device, one rectangle for the
        batch; d_out holds batch x h x w x C bytes (frame f at f * h * w * C)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_region_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch, width,
                                                 height, channels, int(x), int(y), int(w), int(h), _ptr(d_out),
                                                 _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_region_device")

    def decode_regions(self, streams, rects, outs=None):
        """himg_hip_decode_regions_batch: rectangle rects[i] = (x, y, w, h) of stream i at full
        resolution, as one (h_i, w_i, C_i) uint8 array per frame (frames that share the geometry and
        the window size share device launches of up to 256 frames; only each stream's head and the
        block rows its rectangle touches are uploaded).  `outs` (optional) are reusable uint8 buffers."""
        streams = [_as_u8(s_) for s_ in streams]
        rc_ = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(len(streams), 4))
        return self._batch(lib().himg_hip_decode_regions_batch, "decode_regions", streams, outs, _window_bytes(rc_),
                           rc_.ctypes.data)

    def decode_regions_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, origins, w, h,
                              d_out, d_status, stream=0):
        """himg_hip_decode_regions_device: the contract of decode_region_device, with the window
        w x h at origin (x_f, y_f) = origins[f] in frame f (origins: (batch, 2) int32, on the host);
        d_out holds batch x h x w x C bytes (frame f at f * h * w * C)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(batch, 2))
        rc = lib().himg_hip_decode_regions_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch, width,
                                                  height, channels, org.ctypes.data, int(w), int(h), _ptr(d_out),
                                                  _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_regions_device")

    def decode_stream_regions_device(self, d_packed, in_stride, h_sizes, n_streams, width, height, channels,
                                     stream_of, origins, w, h, d_out, d_status, stream=0):
        """himg_hip_decode_stream_regions_device: window k is the w x h rectangle at origins[k] of stream
        stream_of[k] (both on the host; any order, repeats and overlaps allowed); d_out holds
        n_windows x h x w x C bytes (window k at k * h * w * C), d_status n_windows words.  A stream's head
        runs once however many windows name it; every window's bytes and status are decode_regions_device's
        for that stream with that rectangle alone."""
        hs = None if h_sizes is None else np.ascontiguousarray(h_sizes, np.uint32)
        so = None if stream_of is None else np.ascontiguousarray(np.asarray(stream_of, np.int32).ravel())
        org = None if origins is None else np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
        n = 0 if so is None else int(so.size)
        if org is not None and so is not None and org.shape[0] != n:
            raise ValueError("stream_of and origins differ in length")
        rc = lib().himg_hip_decode_stream_regions_device(
            self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data if hs is not None else None, int(n_streams), width,
            height, channels, so.ctypes.data if n else None, org.ctypes.data if org is not None and org.size else None,
            n, int(w), int(h), _ptr(d_out), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_stream_regions_device")

    def decode_stream_regions(self, packed, origins, w, h, out=None):
        """himg_hip_decode_stream_regions_to: n windows of w x h at origins[k] = (x, y) of ONE host stream, as
        ((n, h, w, C) uint8 array, statuses): statuses[k] is 0 or window k's error code, and a failed window's
        pixels are unspecified.  Only the stream's head and the union of the windows' block rows are uploaded
        (stream_regions_peek).  Raises HimgError only where no window could run (a bad stream or rectangle)."""
        packed = _as_u8(packed)
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
        n = org.shape[0]
        st = np.zeros(max(n, 1), np.int32)
        wo, ho, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        geom = _peek(packed)
        if geom:
            cap = n * max(int(w), 0) * max(int(h), 0) * geom[2]
            out = _out_buffer(out, cap)
            dst = out.ctypes.data
        rc = lib().himg_hip_decode_stream_regions_to(self._ctx, packed.ctypes.data, packed.nbytes, n, org.ctypes.data,
                                                     int(w), int(h), dst, cap, st.ctypes.data, C.byref(wo),
                                                     C.byref(ho), C.byref(c))
        if rc != 0 and (wo.value == 0 or rc == HIMG_ERR_CAPACITY):
            self._check(rc, "decode_stream_regions")
        return out.ravel()[: n * ho.value * wo.value * c.value].reshape(n, ho.value, wo.value, c.value), st[:n].copy()

    def open_streams_device(self, d_packed, in_stride, h_sizes, n_streams, width, height, channels,
                            d_head_status=None, stream=0):
        """himg_hip_open_streams_device: the head of every stream once, all its row headers walked once; returns
        an OpenedStreams whose calls decode windows with no parse, LRES chain or walk.  d_packed stays the
        caller's and must stay valid, its payloads unchanged, while the handle lives.  d_head_status (optional):
        n_streams int32 words on the device, each stream's head verdict."""
        hs = None if h_sizes is None else np.ascontiguousarray(h_sizes, np.uint32)
        o = C.c_void_p()
        rc = lib().himg_hip_open_streams_device(self._ctx, _ptr(d_packed), in_stride,
                                                hs.ctypes.data if hs is not None else None, int(n_streams), width, height,
                                                channels, _ptr(d_head_status), C.byref(o), C.c_void_p(stream))
        self._check(rc, "open_streams_device")
        return OpenedStreams(self, o, keep=d_packed)

    def open_stream(self, packed):
        """himg_hip_open_stream_host: one host stream, uploaded whole into memory the handle owns."""
        packed = _as_u8(packed)
        o = C.c_void_p()
        rc = lib().himg_hip_open_stream_host(self._ctx, packed.ctypes.data, packed.nbytes, C.byref(o))
        self._check(rc, "open_stream")
        return OpenedStreams(self, o)

    def decode_regions_tensor_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, origins,
                                     w, h, desc, d_out, d_status, stream=0):
        """himg_hip_decode_regions_tensor_device: the contract of decode_regions_device with the
        planar float output of `desc` (tensor_desc): d_out holds [batch][Co][h][w] elements."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(batch, 2))
        rc = lib().himg_hip_decode_regions_tensor_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch,
                                                         width, height, channels, org.ctypes.data, int(w), int(h),
                                                         C.byref(desc), _ptr(d_out), _ptr(d_status),
                                                         C.c_void_p(stream))
        self._check(rc, "decode_regions_tensor_device")

    def decode_into_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, d_dst, dst,
                           origins, d_status, stream=0):
        """himg_hip_decode_into_device: the contract of decode_device, with frame f's picture written
        at origin (x_f, y_f) = origins[f] of destination picture f of `dst` (dst_desc; frame_pitch 0:
        every frame into ONE picture).  origins: (batch, 2) int32, on the host.  Nothing but the
        pictures' own channel bytes is written."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(batch, 2))
        rc = lib().himg_hip_decode_into_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch, width,
                                               height, channels, _ptr(d_dst), C.byref(dst), org.ctypes.data,
                                               _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_into_device")

    def decode_regions_into_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, src_origins,
                                   w, h, d_dst, dst, dst_origins, d_status, stream=0):
        """himg_hip_decode_regions_into_device: the contract of decode_regions_device (window w x h at
        src_origins[f] of frame f), written at dst_origins[f] of destination picture f of `dst`
        (dst_desc)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        so = np.ascontiguousarray(np.asarray(src_origins, np.int32).reshape(batch, 2))
        do = np.ascontiguousarray(np.asarray(dst_origins, np.int32).reshape(batch, 2))
        rc = lib().himg_hip_decode_regions_into_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch,
                                                       width, height, channels, so.ctypes.data, int(w), int(h),
                                                       _ptr(d_dst), C.byref(dst), do.ctypes.data, _ptr(d_status),
                                                       C.c_void_p(stream))
        self._check(rc, "decode_regions_into_device")

    def decode_into(self, packed, data, dst, x, y):
        """himg_hip_decode_into_to: the picture of the host stream `packed` into the host picture `data`
        (a writable, contiguous uint8 array laid out as `dst` says: dst_desc) at (x, y).  Returns
        (width, height, channels) of the stream."""
        packed = _as_u8(packed)
        if not (isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags.c_contiguous and data.flags.writeable):
            raise HimgError(HIMG_ERR_ARG, "decode_into: data must be a writable contiguous uint8 array")
        # (the array holds the whole picture `dst` describes: the library writes inside that picture only)
        if dst.height < 1 or (dst.height - 1) * dst.row_pitch + dst.width * dst.pixel_stride > data.nbytes:
            raise HimgError(HIMG_ERR_ARG, "decode_into: data is smaller than the picture dst describes")
        w, h, c = C.c_int(), C.c_int(), C.c_int()
        rc = lib().himg_hip_decode_into_to(self._ctx, packed.ctypes.data, packed.nbytes, data.ctypes.data,
                                           C.byref(dst), int(x), int(y), C.byref(w), C.byref(h), C.byref(c))
        self._check(rc, "decode_into")
        return w.value, h.value, c.value

    def decode_scaled(self, packed, scale_log2, out=None):
        """The picture at 1/2 (scale_log2 = 1) or 1/4 (2) scale (himg_hip_decode_scaled_to) as a
        (ceil(H/F), ceil(W/F), C) uint8 array, F = 2 ** scale_log2: the decode the format defines
        at that scale from each tile's lowest-sequency coefficients, not a shrunken decode()."""
        packed = _as_u8(packed)
        wo, ho, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        geom = _peek(packed) if scale_log2 in (1, 2) else None
        if geom:
            ow, oh = scaled_size(geom[0], geom[1], scale_log2)
            cap = ow * oh * geom[2]
            out = _out_buffer(out, cap)
            dst = out.ctypes.data
        rc = lib().himg_hip_decode_scaled_to(self._ctx, packed.ctypes.data, packed.nbytes, int(scale_log2), dst, cap,
                                             C.byref(wo), C.byref(ho), C.byref(c))
        self._check(rc, "decode_scaled")
        return out.ravel()[: ho.value * wo.value * c.value].reshape(ho.value, wo.value, c.value)

    def decode_scaled_batch(self, streams, scale_log2, outs=None):
        """himg_hip_decode_scaled_batch: several streams at 1/2 or 1/4 scale (frames of one
        geometry share device launches of up to 256 frames); `outs` (optional) are reusable uint8
        buffers."""
        def frame_bytes(i, s_):
            geom = _peek(s_) if scale_log2 in (1, 2) else None
            if not geom:
                return 0
            ow, oh = scaled_size(geom[0], geom[1], scale_log2)
            return ow * oh * geom[2]
        return self._batch(lib().himg_hip_decode_scaled_batch, "decode_scaled_batch", [_as_u8(s_) for s_ in streams],
                           outs, frame_bytes, int(scale_log2))

    def decode_scaled_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, scale_log2,
                             d_out, d_status, stream=0):
        """himg_hip_decode_scaled_device: the contract of decode_device; d_out holds
        batch x ceil(H/F) x ceil(W/F) x C bytes, F = 2 ** scale_log2 (frame f at f * oh * ow * C)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_scaled_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch, width,
                                                 height, channels, int(scale_log2), _ptr(d_out), _ptr(d_status),
                                                 C.c_void_p(stream))
        self._check(rc, "decode_scaled_device")

    def decode_pyramid_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, pyramid,
                              d_status, stream=0):
        """himg_hip_decode_pyramid_device: the contract of decode_device with a pyramid_desc() where
        d_out stands there -- level k holds batch x ceil(H/2^k) x ceil(W/2^k) x C bytes; one verdict per
        frame, the full decode's.  pyramid: a PyramidDesc, or None (HIMG_ERR_ARG)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_pyramid_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch, width,
                                                  height, channels, None if pyramid is None else C.addressof(pyramid),
                                                  _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_pyramid_device")

    def decode_pyramid(self, packed, levels=(0, 1, 2, 3)):
        """The picture at 1 / 2^k for every k in `levels` (himg_hip_decode_pyramid_to: one upload, one
        device pass, a download per level) as {level: (ceil(H/2^k), ceil(W/2^k), C) uint8 array}: level 0
        is decode(), 1 and 2 decode_scaled(), 3 preview() -- with the full decode's verdict."""
        packed = _as_u8(packed)
        levels = sorted(set(int(k) for k in levels))
        if any(k < 0 or k > 3 for k in levels):
            raise HimgError(HIMG_ERR_ARG, "decode_pyramid: levels are 0..3")
        geom = _peek(packed)
        outs, dst, cap = {}, (C.c_void_p * 4)(), (C.c_size_t * 4)()
        if geom:
            for k in levels:
                ow, oh = pyramid_size(geom[0], geom[1], k)
                outs[k] = np.empty((oh, ow, geom[2]), np.uint8)
                dst[k], cap[k] = outs[k].ctypes.data, outs[k].nbytes
        w, h, c = C.c_int(), C.c_int(), C.c_int()
        rc = lib().himg_hip_decode_pyramid_to(self._ctx, packed.ctypes.data, packed.nbytes, dst, cap,
                                              C.byref(w), C.byref(h), C.byref(c))
        self._check(rc, "decode_pyramid")
        return outs

    def decode_scaled_region(self, packed, scale_log2, x, y, w, h, out=None):
        """Rectangle (x, y, w, h) of the picture at 1/2 (scale_log2 = 1) or 1/4 (2) scale, in that
        picture's coordinates (himg_hip_decode_scaled_region_to), as an (h, w, C) uint8 array: sample
        (i, j) is sample (y + i, x + j) of decode_scaled().  Only the stream's head and the block
        rows the rectangle touches are uploaded (scaled_region_peek)."""
        packed = _as_u8(packed)
        wo, ho, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        geom = _peek(packed)
        if geom:
            cap = max(int(w), 0) * max(int(h), 0) * geom[2]
            out = _out_buffer(out, cap)
            dst = out.ctypes.data
        rc = lib().himg_hip_decode_scaled_region_to(self._ctx, packed.ctypes.data, packed.nbytes, int(scale_log2), int(x),
                                                    int(y), int(w), int(h), dst, cap, C.byref(wo), C.byref(ho),
                                                    C.byref(c))
        self._check(rc, "decode_scaled_region")
        return out.ravel()[: ho.value * wo.value * c.value].reshape(ho.value, wo.value, c.value)

    def decode_scaled_regions(self, streams, scale_log2, rects, outs=None):
        """himg_hip_decode_scaled_regions_batch: rectangle rects[i] = (x, y, w, h) of stream i's
        picture at 1/2 or 1/4 scale, as one (h_i, w_i, C_i) uint8 array per frame (frames that share
        the geometry and the window size share device launches of up to 256 frames; only each
        stream's head and the block rows its rectangle touches are uploaded).  `outs` (optional) are
        reusable uint8 buffers."""
        streams = [_as_u8(s_) for s_ in streams]
        rc_ = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(len(streams), 4))
        return self._batch(lib().himg_hip_decode_scaled_regions_batch, "decode_scaled_regions", streams, outs,
                           _window_bytes(rc_), int(scale_log2), rc_.ctypes.data)

    def decode_scaled_regions_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, scale_log2,
                                     origins, w, h, d_out, d_status, stream=0):
        """himg_hip_decode_scaled_regions_device: the contract of decode_regions_device at a scale --
        the window w x h at origin (x_f, y_f) = origins[f] of frame f's scaled picture (origins:
        (batch, 2) int32, on the host); d_out holds batch x h x w x C bytes (frame f at f * h * w * C)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(batch, 2))
        rc = lib().himg_hip_decode_scaled_regions_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data, batch,
                                                         width, height, channels, int(scale_log2), org.ctypes.data,
                                                         int(w), int(h), _ptr(d_out), _ptr(d_status),
                                                         C.c_void_p(stream))
        self._check(rc, "decode_scaled_regions_device")

    def get_option(self, option):
        """himg_hip_get_option: the option as the context holds it (names as in set_option)."""
        opt = _OPTIONS[option] if isinstance(option, str) else int(option)
        v = C.c_int(0)
        self._check(lib().himg_hip_get_option(self._ctx, opt, C.byref(v)), "get_option")
        return v.value

    def set_option(self, option, value):
        """himg_hip_set_option; option names: "fix_t2", and the kernel-variant selectors
        "count_wave" / "emit_rows" (-1 = by launch size, 0 / 1 = force; see include/himg_hip.h),
        "count_stretch" (sub-sequences per lane of the wavefront-per-row count kernel: -1, 1, 2, 4, 8)."""
        opt = _OPTIONS[option] if isinstance(option, str) else int(option)
        self._check(lib().himg_hip_set_option(self._ctx, opt, int(value)), "set_option")
        if opt == 1:
            self.fix_t2 = bool(value)   # (the row-sharded decoder's host index follows it, sharded.py)

    # device-resident API -------------------------------------------------------
    def encode_device(self, d_frames, batch, width, height, pixel_stride, channels, quality,
                      use_ycbcr, d_out, out_stride, d_sizes, d_status, stream=0):
        rc = lib().himg_hip_encode_device(self._ctx, _ptr(d_frames), batch, width, height,
                                          pixel_stride, channels, quality, 1 if use_ycbcr else 0,
                                          _ptr(d_out), out_stride, _ptr(d_sizes), _ptr(d_status),
                                          C.c_void_p(stream))
        self._check(rc, "encode_device")

    def encode_device_q(self, d_frames, batch, width, height, pixel_stride, channels, qualities,
                        use_ycbcr, d_out, out_stride, d_sizes, d_status, stream=0):
        """himg_hip_encode_device_q: encode_device with a quality per frame (qualities: `batch` values
        in [0, 100], on the host)."""
        q = np.ascontiguousarray(np.asarray(qualities, np.int32).reshape(batch))
        rc = lib().himg_hip_encode_device_q(self._ctx, _ptr(d_frames), batch, width, height, pixel_stride, channels,
                                            q.ctypes.data, 1 if use_ycbcr else 0, _ptr(d_out), out_stride,
                                            _ptr(d_sizes), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "encode_device_q")

    def encode_windows_device(self, d_src, src, batch, channels, origins, w, h, qualities, use_ycbcr, d_out,
                              out_stride, d_sizes, d_status, stream=0):
        """himg_hip_encode_windows_device: encode_device_q of the w x h window at origin (x_f, y_f) =
        origins[f] of source picture f of `src` (src_desc; frame_pitch 0: every window of one picture).
        origins: (batch, 2) int32 and qualities: `batch` values, both on the host."""
        q = np.ascontiguousarray(np.asarray(qualities, np.int32).reshape(batch))
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(batch, 2))
        rc = lib().himg_hip_encode_windows_device(self._ctx, _ptr(d_src), C.byref(src), batch, channels,
                                                  org.ctypes.data, int(w), int(h), q.ctypes.data,
                                                  1 if use_ycbcr else 0, _ptr(d_out), out_stride, _ptr(d_sizes),
                                                  _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "encode_windows_device")

    def encode_sizes_device(self, d_frames, batch, width, height, pixel_stride, channels, qualities,
                            use_ycbcr, d_sizes, d_status, stream=0):
        """himg_hip_encode_sizes_device: every frame's exact stream size at its quality into d_sizes,
        without writing a stream."""
        q = np.ascontiguousarray(np.asarray(qualities, np.int32).reshape(batch))
        rc = lib().himg_hip_encode_sizes_device(self._ctx, _ptr(d_frames), batch, width, height, pixel_stride,
                                                channels, q.ctypes.data, 1 if use_ycbcr else 0, _ptr(d_sizes),
                                                _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "encode_sizes_device")

    def encode_budget_device(self, d_frames, batch, width, height, pixel_stride, channels, qmin, qmax,
                             use_ycbcr, budgets, d_out, out_stride, d_sizes, d_quality, d_status, stream=0):
        """himg_hip_encode_budget_device: every frame at the quality the search finds for its budget
        (budgets: `batch` byte counts, on the host); d_quality receives the qualities (-1: the
        frame's stream at qmin is larger than its budget)."""
        b = np.ascontiguousarray(np.minimum(np.asarray(budgets, np.uint64), 0xffffffff).astype(np.uint32).reshape(batch))
        rc = lib().himg_hip_encode_budget_device(self._ctx, _ptr(d_frames), batch, width, height, pixel_stride,
                                                 channels, int(qmin), int(qmax), 1 if use_ycbcr else 0,
                                                 b.ctypes.data, _ptr(d_out), out_stride, _ptr(d_sizes),
                                                 _ptr(d_quality), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "encode_budget_device")

    def encode_sse_device(self, d_frames, batch, width, height, pixel_stride, channels, qualities,
                          use_ycbcr, d_sse, d_status, stream=0):
        """himg_hip_encode_sse_device: every frame's exact sum of squared differences between the
        source and the decode of its encode at its quality into d_sse (`batch` 64-bit words), without
        writing a stream."""
        q = np.ascontiguousarray(np.asarray(qualities, np.int32).reshape(batch))
        rc = lib().himg_hip_encode_sse_device(self._ctx, _ptr(d_frames), batch, width, height, pixel_stride,
                                              channels, q.ctypes.data, 1 if use_ycbcr else 0, _ptr(d_sse),
                                              _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "encode_sse_device")

    def encode_target_device(self, d_frames, batch, width, height, pixel_stride, channels, qmin, qmax,
                             use_ycbcr, max_sses, d_out, out_stride, d_sizes, d_quality, d_sse, d_status, stream=0):
        """himg_hip_encode_target_device: every frame at the quality the search finds for its target
        (max_sses: `batch` sums of squared differences, on the host); d_quality receives the qualities
        (-1: the frame misses its target at qmax), d_sse the sums reached."""
        t = np.ascontiguousarray(np.array([min(max(int(x), 0), 2 ** 64 - 1) for x in max_sses], np.uint64).reshape(batch))
        rc = lib().himg_hip_encode_target_device(self._ctx, _ptr(d_frames), batch, width, height, pixel_stride,
                                                 channels, int(qmin), int(qmax), 1 if use_ycbcr else 0,
                                                 t.ctypes.data, _ptr(d_out), out_stride, _ptr(d_sizes),
                                                 _ptr(d_quality), _ptr(d_sse), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "encode_target_device")

    def decode_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, d_out,
                      d_status, stream=0):
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data,
                                          batch, width, height, channels, _ptr(d_out),
                                          _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_device")

    def row_records_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, d_status, stream=0):
        """himg_hip_debug_row_records: the front of decode_device up to the row records, no row kernel;
        read them with debug_read("lane_start" / "lane_off", frame, nbytes, np.uint32, decoder=True)."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_debug_row_records(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data,
                                              batch, width, height, channels, _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "row_records_device")

    def decode_tensor_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, desc, d_out,
                             d_status, stream=0):
        """himg_hip_decode_tensor_device: the contract of decode_device with the planar float output
        of `desc` (tensor_desc): d_out holds [batch][Co][H][W] elements of desc's type."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_tensor_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data,
                                                 batch, width, height, channels, C.byref(desc), _ptr(d_out),
                                                 _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_tensor_device")

    def decode_planes_device(self, d_packed, in_stride, h_sizes, batch, width, height, channels, plane_mask, d_out,
                             d_status, stream=0):
        """himg_hip_decode_planes_device: the contract of decode_device with the stream's own channel
        planes as the output: d_out holds [batch][P][H][W] bytes, P = popcount(plane_mask), the planes
        of the wanted channels (bit c of plane_mask) in ascending order, in front of the colour inverse."""
        hs = np.ascontiguousarray(h_sizes, np.uint32)
        rc = lib().himg_hip_decode_planes_device(self._ctx, _ptr(d_packed), in_stride, hs.ctypes.data,
                                                 batch, width, height, channels, int(plane_mask) & 0xFFFFFFFF,
                                                 _ptr(d_out), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_planes_device")

    def decode_planes(self, packed, plane_mask, out=None):
        """himg_hip_decode_planes_to: the wanted planes of one host stream as a (P, H, W) uint8 array
        (`out` is reused when it has the right size).  Plane 0 of a colour-space-1 stream is its luma
        (peek_format says which colour space a stream has)."""
        packed = _as_u8(packed)
        mask = int(plane_mask) & 0xFFFFFFFF
        w, h, c = C.c_int(), C.c_int(), C.c_int()
        dst, cap = None, 0
        geom = _peek(packed)
        if geom:
            planes = bin(mask & ((1 << geom[2]) - 1)).count("1")
            out = _out_buffer(out, planes * geom[0] * geom[1])
            dst, cap = out.ctypes.data, out.nbytes
        rc = lib().himg_hip_decode_planes_to(self._ctx, packed.ctypes.data, packed.nbytes, mask, dst, cap,
                                             C.byref(w), C.byref(h), C.byref(c))
        self._check(rc, "decode_planes")
        return out.reshape(-1, h.value, w.value)

    def decode_rows_device(self, d_packed, packed_size, width, height, channels, row0, row1,
                           d_out_rows, d_status, stream=0):
        """Block rows [row0, row1) of one frame (row-sharded decode, himg_amd/sharded.py)."""
        rc = lib().himg_hip_decode_rows_device(self._ctx, _ptr(d_packed), int(packed_size), width,
                                               height, channels, row0, row1, _ptr(d_out_rows),
                                               _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_rows_device")

    def decode_index_device(self, d_packed, packed_size, width, height, channels, d_row_index,
                            d_rows_first, d_status, stream=0):
        """Row index of a stream in HBM: [rows] payload offsets + [rows] lengths (uint32) and
        the offset of the first row header (rank 0 of a row-sharded decode)."""
        rc = lib().himg_hip_decode_index_device(self._ctx, _ptr(d_packed), int(packed_size), width, height,
                                                channels, _ptr(d_row_index), _ptr(d_rows_first),
                                                _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_index_device")

    def decode_rows_indexed_device(self, d_packed, packed_size, width, height, channels, row0, row1,
                                   d_row_index, d_out_rows, d_status, stream=0):
        """Block rows [row0, row1) from a buffer that holds only the bytes in front of the first
        row header and these rows' payloads, with the row index supplied."""
        rc = lib().himg_hip_decode_rows_indexed_device(self._ctx, _ptr(d_packed), int(packed_size), width,
                                                       height, channels, row0, row1, _ptr(d_row_index),
                                                       _ptr(d_out_rows), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_rows_indexed_device")

    def decode_head_device(self, d_packed, packed_size, width, height, channels, stream=0):
        """What needs only the head of the stream (container parse, LRES chain, predictor
        inverse); decode_rows_after_head_device follows on the same stream."""
        rc = lib().himg_hip_decode_head_device(self._ctx, _ptr(d_packed), int(packed_size), width, height,
                                               channels, C.c_void_p(stream))
        self._check(rc, "decode_head_device")

    def decode_rows_after_head_device(self, d_packed, packed_size, width, height, channels, row0, row1,
                                      d_row_index, d_out_rows, d_status, stream=0):
        rc = lib().himg_hip_decode_rows_after_head_device(self._ctx, _ptr(d_packed), int(packed_size), width,
                                                          height, channels, row0, row1, _ptr(d_row_index),
                                                          _ptr(d_out_rows), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_rows_after_head_device")

    def decode_first_device(self, d_packed, packed_size, width, height, channels, d_rows_first, d_status,
                            stream=0):
        """Offset of the first FRES row header of a stream in HBM, without the header walk."""
        rc = lib().himg_hip_decode_first_device(self._ctx, _ptr(d_packed), int(packed_size), width, height,
                                                channels, _ptr(d_rows_first), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "decode_first_device")

    def decode_walk_device(self, d_packed, packed_size, width, height, channels, d_row_index, d_rows_first,
                           d_status, stream=0):
        """The row index by the header walk alone, on the context's side stream (beside a head
        phase launched after this call); results valid after decode_walk_wait()."""
        rc = lib().himg_hip_decode_walk_device(self._ctx, _ptr(d_packed), int(packed_size), width, height, channels,
                                               _ptr(d_row_index), _ptr(d_rows_first), _ptr(d_status),
                                               C.c_void_p(stream))
        self._check(rc, "decode_walk_device")

    def decode_walk_ranges_device(self, d_packed, packed_size, width, height, channels, range_end, d_row_index,
                                  d_rows_first, d_range_status, stream=0):
        """himg_hip_decode_walk_ranges_device: the header walk in row ranges on the side stream;
        range k's index entries and verdict are complete after decode_walk_wait_range(k)."""
        ends = (C.c_int * len(range_end))(*[int(x) for x in range_end])
        rc = lib().himg_hip_decode_walk_ranges_device(self._ctx, _ptr(d_packed), int(packed_size), width, height,
                                                      channels, ends, len(range_end), _ptr(d_row_index),
                                                      _ptr(d_rows_first), _ptr(d_range_status), C.c_void_p(stream))
        self._check(rc, "decode_walk_ranges_device")

    def decode_walk_wait_range(self, k):
        self._check(lib().himg_hip_decode_walk_wait_range(self._ctx, int(k)), "decode_walk_wait_range")

    def decode_walk_wait(self):
        self._check(lib().himg_hip_decode_walk_wait(self._ctx), "decode_walk_wait")

    # row-sharded encode (see himg_amd/sharded.py) --------------------------------------
    def shard_stats(self, d_frame_base, width, height, pixel_stride, channels, quality, use_ycbcr,
                    row0, row1, d_hist, d_low_rows, stream=0):
        rc = lib().himg_hip_shard_stats(self._ctx, _ptr(d_frame_base), width, height, pixel_stride,
                                        channels, quality, 1 if use_ycbcr else 0, row0, row1,
                                        _ptr(d_hist), _ptr(d_low_rows), C.c_void_p(stream))
        self._check(rc, "shard_stats")

    def shard_row_bits(self, d_hist_global, d_row_bits, stream=0):
        rc = lib().himg_hip_shard_row_bits(self._ctx, _ptr(d_hist_global), _ptr(d_row_bits),
                                           C.c_void_p(stream))
        self._check(rc, "shard_row_bits")

    def shard_emit(self, d_all_row_bits, d_rel, rel_cap, d_rel_size, stream=0):
        rc = lib().himg_hip_shard_emit(self._ctx, _ptr(d_all_row_bits), _ptr(d_rel), rel_cap,
                                       _ptr(d_rel_size), C.c_void_p(stream))
        self._check(rc, "shard_emit")

    def shard_assemble(self, d_low_full, d_all_row_bits, d_rel, rel_bytes, d_out, out_cap, d_size,
                       d_status, stream=0):
        rc = lib().himg_hip_shard_assemble(self._ctx, _ptr(d_low_full), _ptr(d_all_row_bits),
                                           _ptr(d_rel), rel_bytes, _ptr(d_out), out_cap,
                                           _ptr(d_size), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "shard_assemble")

    def shard_head(self, d_low_full, d_all_row_bits, d_out, out_cap, d_size, d_head, d_status, stream=0):
        rc = lib().himg_hip_shard_head(self._ctx, _ptr(d_low_full), _ptr(d_all_row_bits), _ptr(d_out), out_cap,
                                       _ptr(d_size), _ptr(d_head), _ptr(d_status), C.c_void_p(stream))
        self._check(rc, "shard_head")

    def shard_finish(self, d_out, out_cap, d_size, stream=0):
        rc = lib().himg_hip_shard_finish(self._ctx, _ptr(d_out), out_cap, _ptr(d_size), C.c_void_p(stream))
        self._check(rc, "shard_finish")

    # introspection ---------------------------------------------------------------
    def debug_read(self, what, frame, nbytes, dtype=np.uint8, decoder=False):
        buf = np.empty(nbytes, np.uint8)
        n = C.c_size_t()
        sel = DBG[what] | (DBG_DECODER if decoder else 0)
        rc = lib().himg_hip_debug_read(self._ctx, sel, frame, buf.ctypes.data, nbytes, C.byref(n))
        self._check(rc, "debug_read(%s)" % what)
        return buf[: n.value].view(dtype)

    def debug_trees(self, hists):
        """himg_hip_debug_trees: k_tree alone on n histograms of 261 counts, each in both stream slots of
        its own frame.  Returns codes [n][2][261] u64, lens [n][2][261] u32, trees [n][2][384] u8,
        tree_bytes [n][2] u32 and status [n] i32 (3: a code longer than 32 bits)."""
        h = np.ascontiguousarray(hists, np.uint32).reshape(-1, 261)
        n = h.shape[0]
        codes, lens = np.zeros((n, 2, 261), np.uint64), np.zeros((n, 2, 261), np.uint32)
        trees, nb = np.zeros((n, 2, 384), np.uint8), np.zeros((n, 2), np.uint32)
        status = np.zeros(n, np.int32)
        rc = lib().himg_hip_debug_trees(self._ctx, h.ctypes.data, n, codes.ctypes.data, lens.ctypes.data,
                                        trees.ctypes.data, nb.ctypes.data, status.ctypes.data)
        self._check(rc, "debug_trees")
        return codes, lens, trees, nb, status

    def profile(self, enable):
        lib().himg_hip_profile_enable(self._ctx, 1 if enable else 0)

    def profile_reset(self):
        lib().himg_hip_profile_reset(self._ctx)

    def profile_read(self):
        n = C.c_int()
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        cnt = (C.c_int * 32)()
        rc = lib().himg_hip_profile_read(self._ctx, C.byref(n), names, ms, cnt)
        self._check(rc, "profile_read")
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}


class OpenedStreams:
    """An opened-streams handle (Engine.open_streams_device, Engine.open_stream): the heads' products and the
    rows' records stay on the device between calls.  A context manager; close() waits for the last call."""

    def __init__(self, engine, handle, keep=None):
        self._eng, self._h, self._keep = engine, handle, keep   # (keep: the caller's device buffer stays alive)

    def _ctx(self):
        return self._eng._ctx if self._h else None

    def regions_device(self, stream_of, origins, w, h, d_out, d_status, stream=0, engine=None):
        """himg_hip_opened_regions_device: window k is the w x h rectangle at origins[k] of stream stream_of[k];
        bytes and status words as Engine.decode_stream_regions_device.  engine: the context to call with (the
        one that opened the handle; any other is refused)."""
        so = None if stream_of is None else np.ascontiguousarray(np.asarray(stream_of, np.int32).ravel())
        org = None if origins is None else np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
        n = 0 if so is None else int(so.size)
        if org is not None and so is not None and org.shape[0] != n:
            raise ValueError("stream_of and origins differ in length")
        eng = engine or self._eng
        rc = lib().himg_hip_opened_regions_device(
            eng._ctx if self._h else None, self._h, so.ctypes.data if n else None,
            org.ctypes.data if org is not None and org.size else None, n, int(w), int(h), _ptr(d_out), _ptr(d_status),
            C.c_void_p(stream))
        eng._check(rc, "opened regions_device")

    def regions(self, origins, w, h, stream_of=None, out=None):
        """himg_hip_opened_regions_to: ((n, h, w, C) uint8 array, statuses) as Engine.decode_stream_regions;
        stream_of None: every window of stream 0."""
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
        n = org.shape[0]
        so = None if stream_of is None else np.ascontiguousarray(np.asarray(stream_of, np.int32).ravel())
        c = self.info()["channels"]
        cap = n * max(int(w), 0) * max(int(h), 0) * c
        out = _out_buffer(out, cap)
        st = np.zeros(max(n, 1), np.int32)
        wo, ho, co = C.c_int(), C.c_int(), C.c_int()
        rc = lib().himg_hip_opened_regions_to(self._ctx(), self._h, n, so.ctypes.data if so is not None else None,
                                              org.ctypes.data, int(w), int(h), out.ctypes.data, cap, st.ctypes.data,
                                              C.byref(wo), C.byref(ho), C.byref(co))
        if rc != 0 and (wo.value == 0 or rc == HIMG_ERR_CAPACITY):
            self._eng._check(rc, "opened regions")
        return out.ravel()[:cap].reshape(n, ho.value, wo.value, co.value), st[:n].copy()

    def scaled_regions_device(self, scale_log2, stream_of, origins, w, h, d_out, d_status, stream=None, engine=None):
        """himg_hip_opened_scaled_regions_device: window k is the w x h rectangle at origins[k] of stream
        stream_of[k]'s picture at 1 / 2^scale_log2 (1, 2: bytes and status words as
        Engine.decode_scaled_regions_device on that stream alone; 3: the crop of Engine.preview_device's output and
        the stream's head verdict).  engine: as in regions_device."""
        so = None if stream_of is None else np.ascontiguousarray(np.asarray(stream_of, np.int32).ravel())
        org = None if origins is None else np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
        n = 0 if so is None else int(so.size)
        if org is not None and so is not None and org.shape[0] != n:
            raise ValueError("stream_of and origins differ in length")
        eng = engine or self._eng
        rc = lib().himg_hip_opened_scaled_regions_device(
            eng._ctx if self._h else None, self._h, int(scale_log2), so.ctypes.data if n else None,
            org.ctypes.data if org is not None and org.size else None, n, int(w), int(h), _ptr(d_out), _ptr(d_status),
            C.c_void_p(stream or 0))
        eng._check(rc, "opened scaled_regions_device")

    def scaled_regions(self, scale_log2, origins, w, h, stream_of=None, out=None):
        """himg_hip_opened_scaled_regions_to: ((n, h, w, C) uint8 array, statuses) as regions(), the windows those
        of the picture at 1 / 2^scale_log2; stream_of None: every window of stream 0."""
        org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
        n = org.shape[0]
        so = None if stream_of is None else np.ascontiguousarray(np.asarray(stream_of, np.int32).ravel())
        c = self.info()["channels"]
        cap = n * max(int(w), 0) * max(int(h), 0) * c
        out = _out_buffer(out, cap)
        st = np.zeros(max(n, 1), np.int32)
        wo, ho, co = C.c_int(), C.c_int(), C.c_int()
        rc = lib().himg_hip_opened_scaled_regions_to(self._ctx(), self._h, int(scale_log2), n,
                                                     so.ctypes.data if so is not None else None, org.ctypes.data, int(w),
                                                     int(h), out.ctypes.data, cap, st.ctypes.data, C.byref(wo),
                                                     C.byref(ho), C.byref(co))
        if rc != 0 and (wo.value == 0 or rc == HIMG_ERR_CAPACITY):
            self._eng._check(rc, "opened scaled_regions")
        return out.ravel()[:cap].reshape(n, ho.value, wo.value, co.value), st[:n].copy()

    def info(self):
        """himg_hip_opened_info as a dict: n_streams, width, height, channels, device_bytes, rows_counted."""
        if not self._h:
            raise HimgError(HIMG_ERR_ARG, "the handle is closed")
        n, w, h, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        b, r = C.c_size_t(), C.c_longlong()
        lib().himg_hip_opened_info(self._h, C.byref(n), C.byref(w), C.byref(h), C.byref(c), C.byref(b), C.byref(r))
        return dict(n_streams=n.value, width=w.value, height=h.value, channels=c.value, device_bytes=b.value,
                    rows_counted=r.value)

    def close(self):
        if self._h and self._eng._ctx:
            lib().himg_hip_close_streams(self._eng._ctx, self._h)
        self._h, self._keep = C.c_void_p(), None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def opened_bytes(width, height, channels, n_streams=1):
    """himg_hip_opened_bytes (no GPU): the device bytes an opened-streams handle of this geometry holds."""
    b = C.c_size_t()
    rc = lib().himg_hip_opened_bytes(width, height, channels, n_streams, C.byref(b))
    if rc:
        raise HimgError(rc, "opened_bytes")
    return b.value


class MultiEngine:
    """himg_hip_create_multi: several device slots behind one handle (the same device may
    be named more than once).  encode() / decode() shard ONE frame by block rows over the
    slots; encode_batch() / decode_batch() deal independent frames over them."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._m = C.c_void_p()
        rc = lib().himg_hip_create_multi(devs, len(devices), C.byref(self._m))
        if rc:
            raise HimgError(rc, "himg_hip_create_multi (no usable GPU? there is no CPU fallback)")
        self.devices = list(devices)

    def close(self):
        if self._m:
            lib().himg_hip_destroy_multi(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise HimgError(rc, "%s: %s" % (what, lib().himg_hip_multi_last_error(self._m).decode()))

    def set_option(self, option, value):
        opt = {"fix_t2": 1}[option] if isinstance(option, str) else int(option)
        self._check(lib().himg_hip_multi_set_option(self._m, opt, int(value)), "set_option")

    def encode(self, img, quality=50, use_ycbcr=True, channels=None, pixel_stride=None):
        """channels / pixel_stride as in Engine.encode: the image's last axis where not given."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w, ch, stride = _image_geom(img, channels, pixel_stride)
        out, n = C.c_void_p(), C.c_size_t()
        rc = lib().himg_hip_multi_encode(self._m, img.ctypes.data, w, h, stride, ch, quality, 1 if use_ycbcr else 0,
                                         C.byref(out), C.byref(n))
        self._check(rc, "multi_encode")
        a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (n.value,)).copy()
        lib().himg_hip_free(out)
        return a

    def decode(self, packed):
        packed = np.ascontiguousarray(np.frombuffer(packed, np.uint8) if isinstance(packed, (bytes, bytearray)) else packed)
        out = C.c_void_p()
        w, h, c = C.c_int(), C.c_int(), C.c_int()
        rc = lib().himg_hip_multi_decode(self._m, packed.ctypes.data, packed.nbytes, C.byref(out), C.byref(w),
                                         C.byref(h), C.byref(c))
        self._check(rc, "multi_decode")
        n = w.value * h.value * c.value
        a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (n,)).copy().reshape(h.value, w.value, c.value)
        lib().himg_hip_free(out)
        return a

    def encode_batch(self, frames, quality=50, use_ycbcr=True):
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        n = len(frames)
        h, w = frames[0].shape[:2]
        ch = frames[0].shape[2] if frames[0].ndim == 3 else 1
        cap = max_packed_size(w, h, ch)
        outs = [np.empty(cap, np.uint8) for _ in range(n)]
        src = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
        sizes = (C.c_size_t * n)()
        rc = lib().himg_hip_multi_encode_batch(self._m, src, n, w, h, ch, ch, quality, 1 if use_ycbcr else 0,
                                               dst, caps, sizes)
        self._check(rc, "multi_encode_batch")
        return [o[: sizes[i]] for i, o in enumerate(outs)]

    def decode_batch(self, streams):
        streams = [np.ascontiguousarray(s, np.uint8) for s in streams]
        n = len(streams)
        outs = []
        for s_ in streams:
            w, h, c = C.c_int(), C.c_int(), C.c_int()
            ok = lib().himg_hip_peek(s_.ctypes.data, s_.nbytes, C.byref(w), C.byref(h), C.byref(c)) == HIMG_OK
            outs.append(np.empty(w.value * h.value * c.value if ok else 1, np.uint8))
        src = (C.c_void_p * n)(*[s_.ctypes.data for s_ in streams])
        szs = (C.c_size_t * n)(*[s_.nbytes for s_ in streams])
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
        ws, hs, cs = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        rc = lib().himg_hip_multi_decode_batch(self._m, src, szs, n, dst, caps, ws, hs, cs)
        self._check(rc, "multi_decode_batch")
        return [o[: ws[i] * hs[i] * cs[i]].reshape(hs[i], ws[i], cs[i]) for i, o in enumerate(outs)]


def preview_peek(packed, avail=None, packed_size=None):
    """himg_hip_preview_peek (no GPU): (preview width, preview height, channels, head_bytes)
    of a stream of which `avail` bytes (default: all of `packed`) are present; packed_size is
    the whole stream's size (default: len(packed)).  Raises HimgError (code HIMG_ERR_FORMAT /
    HIMG_ERR_CAPACITY / HIMG_ERR_UNSUPPORTED); on HIMG_ERR_CAPACITY its `head_bytes` is set
    (0 when the LRES header was not reached)."""
    a = _as_u8(packed)
    avail = a.nbytes if avail is None else min(int(avail), a.nbytes)
    size = a.nbytes if packed_size is None else int(packed_size)
    pw, ph, c, hb = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = lib().himg_hip_preview_peek(a.ctypes.data, avail, size, C.byref(pw), C.byref(ph), C.byref(c), C.byref(hb))
    if rc != 0:
        e = HimgError(rc, "preview_peek")
        e.head_bytes = hb.value
        raise e
    return pw.value, ph.value, c.value, hb.value


def scaled_size(w, h, scale_log2):
    """himg_hip_scaled_size (no GPU): (ow, oh) = (ceil(w / F), ceil(h / F)), F = 2 ** scale_log2,
    scale_log2 1 or 2.  Raises HimgError (HIMG_ERR_ARG) for another scale or a non-positive size."""
    ow, oh = C.c_int(), C.c_int()
    rc = lib().himg_hip_scaled_size(int(w), int(h), int(scale_log2), C.byref(ow), C.byref(oh))
    if rc != 0:
        raise HimgError(rc, "scaled_size")
    return ow.value, oh.value


def pyramid_size(width, height, level):
    """himg_hip_pyramid_size (no GPU): (ow, oh) = (ceil(width / 2^level), ceil(height / 2^level)),
    level 0..3.  Raises HimgError (HIMG_ERR_ARG) for another level or a non-positive size."""
    ow, oh = C.c_int(), C.c_int()
    rc = lib().himg_hip_pyramid_size(int(width), int(height), int(level), C.byref(ow), C.byref(oh))
    if rc != 0:
        raise HimgError(rc, "pyramid_size")
    return ow.value, oh.value


class PyramidDesc(C.Structure):
    """himg_hip_pyramid."""
    _fields_ = [("level", C.c_void_p * 4)]


def pyramid_desc(level0=None, level1=None, level2=None, level3=None):
    """A himg_hip_pyramid: the device buffers (torch tensors or addresses) of levels 0..3; None = the
    level is not wanted."""
    d = PyramidDesc()
    for k, x in enumerate((level0, level1, level2, level3)):
        d.level[k] = _ptr(x).value
    return d


class TensorDesc(C.Structure):
    """himg_hip_tensor_desc."""
    _fields_ = [("dtype", C.c_int), ("out_channels", C.c_int), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


def _tensor_dtype(dtype):
    if isinstance(dtype, (int, np.integer)):
        return int(dtype)
    import torch
    table = {torch.float32: HIMG_DT_F32, torch.float16: HIMG_DT_F16, torch.bfloat16: HIMG_DT_BF16}
    if dtype not in table:
        raise ValueError("tensor_desc: dtype must be HIMG_DT_* or torch.float32 / float16 / bfloat16")
    return table[dtype]


def tensor_desc(dtype, out_channels, mean=None, std=None, scale=None, bias=None):
    """A himg_hip_tensor_desc: element = cvt(fma(p, scale[c], bias[c])) of byte p, planar output of the
    first out_channels channels.  dtype: HIMG_DT_* or torch.float32 / float16 / bfloat16.  With
    mean / std (per channel, for pixels scaled to 0..1): scale = 1 / (255 std), bias = -mean / std,
    computed in double and rounded once to float32.  Otherwise scale (default 1) and bias (default 0)
    per channel.  The library validates the descriptor (tensor_bytes, the decode calls)."""
    d = TensorDesc()
    d.dtype = _tensor_dtype(dtype)
    d.out_channels = int(out_channels)
    n = min(max(d.out_channels, 0), 4)
    if mean is not None or std is not None:
        if scale is not None or bias is not None:
            raise ValueError("tensor_desc: mean / std or scale / bias, not both")
        m = [0.0] * n if mean is None else [float(v) for v in mean]
        sd = [1.0] * n if std is None else [float(v) for v in std]
        sc = [1.0 / (255.0 * sd[c]) for c in range(n)]
        bi = [-m[c] / sd[c] for c in range(n)]
    else:
        sc = [1.0] * n if scale is None else [float(v) for v in scale]
        bi = [0.0] * n if bias is None else [float(v) for v in bias]
    for c in range(min(n, len(sc))):
        d.scale[c] = float(np.float32(sc[c]))
    for c in range(min(n, len(bi))):
        d.bias[c] = float(np.float32(bi[c]))
    return d


def tensor_bytes(desc, channels, w, h):
    """himg_hip_tensor_bytes (no GPU): bytes per frame of the [Co][h][w] output of `desc` for a
    picture of `channels` channels.  Raises HimgError (HIMG_ERR_ARG) for a descriptor the decode
    calls reject: an unknown dtype, out_channels outside 1..channels, a non-finite used scale / bias."""
    n = C.c_size_t()
    rc = lib().himg_hip_tensor_bytes(C.byref(desc), int(channels), int(w), int(h), C.byref(n))
    if rc != 0:
        raise HimgError(rc, "tensor_bytes")
    return n.value


def planes_bytes(channels, plane_mask, w, h):
    """himg_hip_planes_bytes (no GPU): bytes per frame of the [P][h][w] planes output for `plane_mask`
    of a stream of `channels` channels.  Raises HimgError (HIMG_ERR_ARG) for what the decode calls
    reject: mask 0, a bit at or above channels, channels outside 1..4, a non-positive size."""
    n = C.c_size_t()
    rc = lib().himg_hip_planes_bytes(int(channels), int(plane_mask) & 0xFFFFFFFF, int(w), int(h), C.byref(n))
    if rc != 0:
        raise HimgError(rc, "planes_bytes")
    return n.value


def peek_format(packed):
    """himg_hip_peek_format (no GPU): (width, height, channels, colour_space) of a stream; colour
    space 1: channels 0..2 of a stream of three or four channels are Y, Cb, Cr.  Raises HimgError
    (HIMG_ERR_FORMAT / HIMG_ERR_UNSUPPORTED)."""
    a = _as_u8(packed)
    w, h, c, cs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().himg_hip_peek_format(a.ctypes.data, a.nbytes, C.byref(w), C.byref(h), C.byref(c), C.byref(cs))
    if rc != 0:
        raise HimgError(rc, "peek_format")
    return w.value, h.value, c.value, cs.value


class SrcDesc(C.Structure):
    """himg_hip_src."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("pixel_stride", C.c_int), ("row_pitch", C.c_size_t),
                ("frame_pitch", C.c_size_t)]


def src_desc(width, height, pixel_stride, row_pitch=None, frame_pitch=None):
    """A himg_hip_src: pictures of width x height pixels, pixel_stride bytes per pixel, rows row_pitch
    bytes apart (default: packed) and pictures frame_pitch bytes apart (default: height * row_pitch;
    0: every window of a call reads ONE picture).  The library validates it (windows_extent, the
    encode calls)."""
    d = SrcDesc()
    d.width, d.height, d.pixel_stride = int(width), int(height), int(pixel_stride)
    d.row_pitch = int(width) * int(pixel_stride) if row_pitch is None else int(row_pitch)
    d.frame_pitch = int(height) * d.row_pitch if frame_pitch is None else int(frame_pitch)
    return d


def windows_extent(src, channels, origins, w, h):
    """himg_hip_windows_extent (no GPU): the bytes of the source buffer that the w x h windows at
    `origins` ((batch, 2): x_f, y_f) of `src` reach -- nothing at or beyond is read.  Raises HimgError
    (HIMG_ERR_ARG) for a descriptor or a window that encode_windows_device rejects."""
    org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
    n = C.c_size_t()
    rc = lib().himg_hip_windows_extent(C.byref(src), int(channels), len(org), org.ctypes.data, int(w), int(h),
                                       C.byref(n))
    if rc != 0:
        raise HimgError(rc, "windows_extent")
    return n.value


class DstDesc(C.Structure):
    """himg_hip_dst."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("pixel_stride", C.c_int), ("row_pitch", C.c_size_t),
                ("frame_pitch", C.c_size_t)]


def dst_desc(width, height, pixel_stride, row_pitch=None, frame_pitch=None):
    """A himg_hip_dst: destination pictures of width x height pixels, pixel_stride bytes per pixel, rows
    row_pitch bytes apart (default: packed) and pictures frame_pitch bytes apart (default:
    height * row_pitch; 0: every window of a call lies in ONE picture).  The library validates it
    (dst_extent, the decode_into calls)."""
    d = DstDesc()
    d.width, d.height, d.pixel_stride = int(width), int(height), int(pixel_stride)
    d.row_pitch = int(width) * int(pixel_stride) if row_pitch is None else int(row_pitch)
    d.frame_pitch = int(height) * d.row_pitch if frame_pitch is None else int(frame_pitch)
    return d


def dst_extent(dst, channels, origins, w, h):
    """himg_hip_dst_extent (no GPU): the bytes of the destination buffer that the w x h windows at
    `origins` ((batch, 2): x_f, y_f) of `dst` reach -- nothing at or beyond is written.  Raises
    HimgError (HIMG_ERR_ARG) for a descriptor or a window that the decode_into calls reject."""
    org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
    n = C.c_size_t()
    rc = lib().himg_hip_dst_extent(C.byref(dst), int(channels), len(org), org.ctypes.data, int(w), int(h),
                                   C.byref(n))
    if rc != 0:
        raise HimgError(rc, "dst_extent")
    return n.value


class RegionPlan(C.Structure):
    """himg_hip_region_plan."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("num_channels", C.c_int), ("row0", C.c_int),
                ("row1", C.c_int), ("head_bytes", C.c_size_t), ("rows_begin", C.c_size_t), ("rows_end", C.c_size_t)]


def region_peek(packed, x, y, w, h, fix_t2=False):
    """himg_hip_region_peek (no GPU): the plan of rectangle (x, y, w, h) as a dict -- width,
    height, num_channels, row0, row1, head_bytes, rows_begin, rows_end.  Raises HimgError
    (HIMG_ERR_ARG for a bad rectangle, HIMG_ERR_FORMAT / HIMG_ERR_UNSUPPORTED as index_host)."""
    a = _as_u8(packed)
    plan = RegionPlan()
    rc = lib().himg_hip_region_peek(a.ctypes.data, a.nbytes, 1 if fix_t2 else 0, int(x), int(y), int(w), int(h),
                                    C.byref(plan))
    if rc != 0:
        raise HimgError(rc, "region_peek")
    return {k: getattr(plan, k) for k, _ in RegionPlan._fields_}


def stream_regions_peek(packed, origins, w, h, fix_t2=False):
    """himg_hip_stream_regions_peek (no GPU): (plans, ranges) for n windows of w x h at origins[k] = (x, y)
    of one stream.  plans[k] is region_peek's dict for window k, or its int error code where it has no plan
    (HIMG_ERR_ARG for a bad rectangle, HIMG_ERR_FORMAT where the header chain breaks before its last row);
    ranges is the sorted, disjoint list of (begin, end) byte ranges a caller must have present:
    [0, head_bytes) and the union of the planned windows' [rows_begin, rows_end)."""
    a = _as_u8(packed)
    org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
    n = org.shape[0]
    plans = (RegionPlan * max(n, 1))()
    rng = np.zeros(2 * (n + 1), np.uintp)
    nr = C.c_int(0)
    rc = lib().himg_hip_stream_regions_peek(a.ctypes.data, a.nbytes, 1 if fix_t2 else 0, n, org.ctypes.data, int(w),
                                            int(h), plans, rng.ctypes.data, C.byref(nr))
    if n < 1:
        raise HimgError(rc, "stream_regions_peek")
    out = [{k: getattr(p, k) for k, _ in RegionPlan._fields_} if p.row1 > 0 else int(p.row0) for p in plans[:n]]
    return out, [(int(rng[2 * i]), int(rng[2 * i + 1])) for i in range(nr.value)]


class PrefixPlan(C.Structure):
    """himg_hip_prefix_plan."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("num_channels", C.c_int), ("rows", C.c_int),
                ("rows_complete", C.c_int), ("packed_size", C.c_size_t), ("head_bytes", C.c_size_t),
                ("used_bytes", C.c_size_t), ("next_bytes", C.c_size_t)]


def prefix_peek(packed, avail=None, fix_t2=False):
    """himg_hip_prefix_peek (no GPU): the plan of a stream of which the first `avail` bytes (default:
    all of `packed`; more than it holds: ValueError) are present, as a dict -- width, height, num_channels, rows, rows_complete,
    packed_size, head_bytes, used_bytes, next_bytes.  Raises HimgError (HIMG_ERR_CAPACITY for a
    prefix that ends before the first row header, else as region_peek); its `plan` holds what the walk
    had reached."""
    a = _as_u8(packed)
    avail = a.nbytes if avail is None else int(avail)
    if not 0 <= avail <= a.nbytes:
        raise ValueError("prefix_peek: avail = %d, but `packed` holds %d bytes" % (avail, a.nbytes))
    plan = PrefixPlan()
    rc = lib().himg_hip_prefix_peek(a.ctypes.data, avail, 1 if fix_t2 else 0, C.byref(plan))
    d = {k: getattr(plan, k) for k, _ in PrefixPlan._fields_}
    if rc != 0:
        e = HimgError(rc, "prefix_peek")
        e.plan = d
        raise e
    return d


class PrefixState(C.Structure):
    """himg_hip_prefix_state."""
    _fields_ = [("started", C.c_uint32), ("rows_done", C.c_int32), ("walk_pos", C.c_uint32),
                ("avail_seen", C.c_uint32)]


PREFIX_STATE_DTYPE = np.dtype([("started", "<u4"), ("rows_done", "<i4"), ("walk_pos", "<u4"), ("avail_seen", "<u4")])


def prefix_states(n):
    """n fresh himg_hip_prefix_state as a zeroed structured array (16 bytes each): upload its bytes for
    decode_prefix_more_device, or pass a one-element slice of it to decode_prefix_more / prefix_peek_from."""
    return np.zeros(int(n), PREFIX_STATE_DTYPE)


def _state_view(state):
    if not (isinstance(state, np.ndarray) and state.dtype == PREFIX_STATE_DTYPE and state.size == 1
            and state.flags["C_CONTIGUOUS"] and state.flags["WRITEABLE"]):
        raise TypeError("a prefix state is a PrefixState or a one-element slice of prefix_states()")
    return state


def prefix_peek_from(packed, state, avail=None, fix_t2=False):
    """himg_hip_prefix_peek_from (no GPU): prefix_peek's dict, reached by resuming the row walk at `state`
    (a PrefixState or a one-element slice of prefix_states(); not changed).  Raises HimgError as
    prefix_peek does, and with HIMG_ERR_ARG for a state that cannot belong to these bytes."""
    a = _as_u8(packed)
    avail = a.nbytes if avail is None else int(avail)
    if not 0 <= avail <= a.nbytes:
        raise ValueError("prefix_peek_from: avail = %d, but `packed` holds %d bytes" % (avail, a.nbytes))
    st = state if isinstance(state, PrefixState) else PrefixState.from_buffer(_state_view(state))
    plan = PrefixPlan()
    rc = lib().himg_hip_prefix_peek_from(a.ctypes.data, avail, 1 if fix_t2 else 0, C.addressof(st), C.byref(plan))
    d = {k: getattr(plan, k) for k, _ in PrefixPlan._fields_}
    if rc != 0:
        e = HimgError(rc, "prefix_peek_from")
        e.plan = d
        raise e
    return d


def scaled_region_peek(packed, scale_log2, x, y, w, h, fix_t2=False):
    """himg_hip_scaled_region_peek (no GPU): the plan of rectangle (x, y, w, h) of the picture at
    1/2 (scale_log2 = 1) or 1/4 (2) scale, as region_peek's dict: it is region_peek of the
    full-resolution rectangle (F x, F y, min(F w, W - F x), min(F h, H - F y)), F = 2 ** scale_log2.
    Raises HimgError (HIMG_ERR_ARG for a bad rectangle or another scale, else as region_peek)."""
    a = _as_u8(packed)
    plan = RegionPlan()
    rc = lib().himg_hip_scaled_region_peek(a.ctypes.data, a.nbytes, 1 if fix_t2 else 0, int(scale_log2), int(x),
                                           int(y), int(w), int(h), C.byref(plan))
    if rc != 0:
        raise HimgError(rc, "scaled_region_peek")
    return {k: getattr(plan, k) for k, _ in RegionPlan._fields_}


def _image_geom(img, channels=None, pixel_stride=None):
    """(h, w, channels, pixel stride) of an image array: its last axis (1 without one) where not given."""
    last = img.shape[2] if img.ndim == 3 else 1
    return img.shape[0], img.shape[1], last if channels is None else channels, last if pixel_stride is None else pixel_stride


def _as_u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, np.uint8)


def _peek(a):
    """himg_hip_peek of a uint8 array: (width, height, channels), or None for a stream it rejects."""
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    if lib().himg_hip_peek(a.ctypes.data, a.nbytes, C.byref(w), C.byref(h), C.byref(c)) != HIMG_OK:
        return None
    return w.value, h.value, c.value


def _out_buffer(out, n):
    """The output buffer of a single-stream decode of n bytes: `out` when it fits, else a new array."""
    if out is None or out.nbytes != n or not out.flags["C_CONTIGUOUS"] or out.dtype != np.uint8:
        out = np.empty(max(n, 1), np.uint8)
    return out


def _window_bytes(rects):
    """frame_bytes (Engine._batch) of window decodes: rects[i] = (x, y, w, h)."""
    def frame_bytes(i, s_):
        geom = _peek(s_)
        return geom and max(int(rects[i][2]), 0) * max(int(rects[i][3]), 0) * geom[2]
    return frame_bytes


def index_host(packed, fix_t2=False):
    """Row index of a stream in host memory (no GPU): (width, height, channels, offsets
    uint32[rows], lengths uint32[rows], rows_first).  Raises HimgError on a stream whose
    container or row headers the decoder would reject."""
    a = np.ascontiguousarray(packed, np.uint8)
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib().himg_hip_peek(a.ctypes.data, a.size, C.byref(w), C.byref(h), C.byref(c))
    if rc != 0:
        raise HimgError(rc, "index_host: not a HIMG stream")
    rows = (h.value + 7) // 8
    idx = np.zeros(2 * rows, np.uint32)
    first = C.c_uint32()
    rc = lib().himg_hip_index_host(a.ctypes.data, a.size, 1 if fix_t2 else 0, C.byref(w), C.byref(h),
                                   C.byref(c), idx.ctypes.data, rows, C.byref(first))
    if rc != 0:
        raise HimgError(rc, "index_host")
    return w.value, h.value, c.value, idx[:rows], idx[rows:], first.value


def _ptr(x):
    """Device pointer of a torch tensor, or a raw integer address."""
    if x is None:
        return C.c_void_p(0)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))
