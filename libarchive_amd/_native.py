"""ctypes bindings of the native libraries (libla_gpu.so, libla_host.so).

Mirrors include/la_gpu.h and include/la_host.h one to one.  No compute happens
in Python; a missing library raises NativeLibraryMissing (never a fallback).
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# LA_GPU_LIB selects a diagnostic build of the data plane (tools/exp_*.sh) without touching the shipped file
GPU_LIB_PATH = os.environ.get("LA_GPU_LIB") or os.path.join(_PKG, "csrc", "libla_gpu.so")
HOST_LIB_PATH = os.path.join(_PKG, "host", "libla_host.so")

LA_OK = 0

# struct la_lz4_block / la_lz4_frame / la_hash_job / la_batch_summary (include/la_gpu.h)
LZ4_BLOCK_DTYPE = np.dtype([("src_off", "<u8"), ("src_len", "<u4"), ("dst_cap", "<u4"),
                            ("flags", "<u4"), ("block_sum", "<u4")])
LZ4_FRAME_DTYPE = np.dtype([("desc_off", "<u8"), ("desc_len", "<u4"), ("first_block", "<u4"),
                            ("n_blocks", "<u4"), ("flags", "<u4"), ("content_sum", "<u4"),
                            ("reserved", "<u4")])
HASH_JOB_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("seed", "<u4")])
SUMMARY_DTYPE = np.dtype([("total_out", "<u8"), ("n_bad_units", "<u4"), ("n_bad_frames", "<u4"),
                          ("first_bad_unit", "<u4"), ("first_bad_frame", "<u4"),
                          ("first_zero_unit", "<u4"), ("reserved", "<u4")])
GZ_MEMBER_DTYPE = np.dtype([("src_off", "<u8"), ("src_len", "<u4"), ("dst_cap", "<u4"), ("dst_off", "<u8")])
GZ_RESULT_DTYPE = np.dtype([("status", "<u4"), ("out_len", "<u4"), ("consumed", "<u4"), ("crc32", "<u4")])
assert LZ4_BLOCK_DTYPE.itemsize == 24 and LZ4_FRAME_DTYPE.itemsize == 32
assert HASH_JOB_DTYPE.itemsize == 16 and SUMMARY_DTYPE.itemsize == 32

LA_LZ4B_STORED, LA_LZ4B_CHECKSUM, LA_LZ4B_DEPENDENT, LA_LZ4B_FIRST = 1, 2, 4, 8
LA_LZ4F_CONTENT_SUM, LA_LZ4F_HEADER_SUM, LA_LZ4F_CONT, LA_LZ4F_OPEN, LA_LZ4F_HASHED = 1, 2, 4, 8, 16
LA_LZ4_OPT_GENERAL_ONLY, LA_LZ4_OPT_NO_VERIFY, LA_LZ4_OPT_PARSE_V1, LA_LZ4_OPT_EXPAND_INORDER = 1, 2, 4, 8
LA_LZ4_OPT_SEARCH_IN_EXPAND = 16
LA_LZ4_OPT_SPLIT_SMALL = 32
LA_GPU_ABI_VERSION = 3
LA_ST_OK, LA_ST_GZ_DATA, LA_ST_GZ_TRUNCATED, LA_ST_GZ_OUT_FULL, LA_ST_GZ_NO_TRAILER = 0, 5, 6, 9, 10
LA_ST_GZ_PIECE_END, LA_ST_GZ_NEEDS_HISTORY = 18, 19     # LA_GZ_OPT_PIECES only
(LA_GZ_OPT_NO_VERIFY, LA_GZ_OPT_WAVE_KERNEL, LA_GZ_OPT_LANE_KERNEL, LA_GZ_OPT_TWO_PHASE, LA_GZ_OPT_RAW,
 LA_GZ_OPT_EXPAND_INORDER, LA_GZ_OPT_PIECES) = 1, 2, 4, 8, 16, 32, 64
LA_GZ_OPT_CHAIN = 128      # with LA_GZ_OPT_PIECES: the pieces depend on each other, output is packed
LA_GZ_OPT_BLOCK_STARTS = 256        # with PIECES | CHAIN and one span: the device finds the block starts itself
LA_GZ_OPT_START_BIT_SHIFT = 16      # the span's first bit, 0..7, in bits 16..18 of the options

(LA_END_EOF, LA_END_TRUNCATED, LA_END_MALFORMED, LA_END_MALFORMED_SKIP, LA_END_EMPTY_FRAME,
 LA_END_NEED_MORE, LA_END_GZ_NO_TRAILER, LA_END_GZ_TOO_LARGE) = range(8)


class NativeLibraryMissing(RuntimeError):
    pass


class _Lz4BatchC(C.Structure):
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("d_blocks", C.c_void_p), ("n_blocks", C.c_uint32),
        ("d_frames", C.c_void_p), ("n_frames", C.c_uint32),
        ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64),
        ("d_out_len", C.c_void_p), ("d_dst_off", C.c_void_p),
        ("d_block_status", C.c_void_p), ("d_frame_status", C.c_void_p),
        ("d_summary", C.c_void_p),
        ("options", C.c_uint32), ("hist_len", C.c_uint32),
        ("d_carry_in", C.c_void_p), ("d_carry_out", C.c_void_p),   # content hash across batches (NULL here)
    ]


class _Lz4cBatchC(C.Structure):
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("block_size", C.c_uint32), ("blocks_per_frame", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
        ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p),
    ]


LA_LZ4C_BLOCK_SUM, LA_LZ4C_CONTENT_SUM = 1, 2


class _ZstdcBatchC(C.Structure):
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("block_size", C.c_uint32), ("blocks_per_frame", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
        ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p),
    ]


LA_ZSTDC_CHECKSUM, LA_ZSTDC_RAW_LITERALS = 1, 2
LA_ZSTDC_FULL_ALPHABET, LA_ZSTDC_FIT_TABLES = 4, 8
LA_ZSTD_OPT_NO_VERIFY, LA_ZSTD_OPT_LANE_KERNEL, LA_ZSTD_OPT_BLOCK_PARALLEL = 1, 2, 4     # la_zstd_batch.options


class _Bz2cBatchC(C.Structure):     # la_bz2c_batch
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("level", C.c_uint32), ("flags", C.c_uint32),
        ("d_state", C.c_void_p),
        ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p),
    ]


LA_BZ2C_FIRST, LA_BZ2C_LAST = 1, 2
BZ2C_STATE_DTYPE = np.dtype([("crc", "<u4"), ("nbits", "<u4"), ("bits", "<u4"), ("reserved", "<u4")])

# bzip2 (la_bz2_cand, la_bz2_result, la_bz2_state, la_bz2_batch)
BZ2_CAND_DTYPE = np.dtype([("bit_off", "<u8"), ("kind", "<u4"), ("reserved", "<u4")])
BZ2_RESULT_DTYPE = np.dtype([("status", "<u4"), ("level", "<u4"), ("out_len", "<u8"), ("end_bit", "<u8"), ("dst_off", "<u8"),
                             ("crc", "<u4"), ("stored_crc", "<u4")])
BZ2_STATE_DTYPE = np.dtype([("open", "<u4"), ("level", "<u4"), ("crc", "<u4"), ("stop", "<u4"), ("start_bit", "<u8"),
                            ("total_out", "<u8"), ("n_taken", "<u4"), ("stop_entry", "<u4"), ("first_bad", "<u4"),
                            ("reserved", "<u4")])
LA_BZ2_KIND_BLOCK, LA_BZ2_KIND_END = 0, 1
LA_BZ2_MEASURE, LA_BZ2_EMIT = 0, 1
LA_BZ2_OPT_SERIAL_CHASE = 1
LA_BZ2_STOP_TABLE, LA_BZ2_STOP_ENTRY, LA_BZ2_STOP_BID, LA_BZ2_STOP_SHORT, LA_BZ2_STOP_LEVEL = 0, 1, 2, 3, 4
LA_ST_BZ2_DATA, LA_ST_BZ2_TRUNCATED, LA_ST_BZ2_BAD_CRC, LA_ST_BZ2_REFUTED, LA_ST_BZ2_RANDOMISED = 20, 21, 22, 23, 24


# xz (la_xz_block, la_xz_result, la_xz_batch)
XZ_BLOCK_DTYPE = np.dtype([("src_off", "<u8"), ("comp_size", "<u8"), ("uncomp_size", "<u8"), ("dst_off", "<u8"), ("dst_cap", "<u8"),
                           ("check_off", "<u8"), ("dict_size", "<u4"), ("check_id", "<u4")])
XZ_RESULT_DTYPE = np.dtype([("status", "<u4"), ("reserved", "<u4"), ("out_len", "<u8"), ("consumed", "<u8"), ("valid", "<u8")])
XZ_CHAIN_DTYPE = np.dtype([("count", "<u4"), ("id", "<u4", (3,)), ("prop", "<u4", (3,)), ("reserved", "<u4")])     # la_xz_chain
LA_XZ_BATCH_CHAINS = 1          # la_xz_batch.reserved: d_blocks[n] is followed by la_xz_chain chains[n]
LA_XZ_UNKNOWN = 0xFFFFFFFFFFFFFFFF
(LA_ST_XZ_DATA, LA_ST_XZ_LZMA, LA_ST_XZ_TRUNCATED, LA_ST_XZ_SIZE, LA_ST_XZ_BAD_CHECK, LA_ST_XZ_PADDING,
 LA_ST_XZ_OUT_FULL) = 25, 26, 27, 28, 29, 30, 31


class _XzBatchC(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("d_blocks", C.c_void_p), ("n", C.c_uint32),
                ("reserved", C.c_uint32), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("d_results", C.c_void_p)]


class _XzcBatchC(C.Structure):      # la_xzc_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("level", C.c_uint32), ("flags", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p)]


LA_XZC_FIRST = 1
LA_XZC_BLOCK_BYTES, LA_XZC_CHUNK_BYTES = 1 << 20, 1 << 16

# lzip (la_lzip_member, la_lzip_result, la_lzip_batch)
LZIP_MEMBER_DTYPE = np.dtype([("src_off", "<u8"), ("src_end", "<u8"), ("data_size", "<u8"), ("dst_off", "<u8"), ("dst_cap", "<u8"),
                              ("dict_size", "<u4"), ("crc32", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
LZIP_RESULT_DTYPE = np.dtype([("status", "<u4"), ("crc32", "<u4"), ("out_len", "<u8"), ("consumed", "<u8"), ("valid", "<u8")])
LA_LZIP_UNKNOWN = 0xFFFFFFFFFFFFFFFF
LA_LZIP_HAS_CRC = 1
(LA_ST_LZIP_DATA, LA_ST_LZIP_SRC_END, LA_ST_LZIP_TRUNCATED, LA_ST_LZIP_EARLY_END, LA_ST_LZIP_SIZE_OVER, LA_ST_LZIP_OUT_FULL,
 LA_ST_LZIP_BAD_SIZE, LA_ST_LZIP_BAD_CRC, LA_ST_LZIP_REFUSED) = 32, 33, 34, 35, 36, 37, 38, 39, 40


class _LzipBatchC(C.Structure):     # la_lzip_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("d_members", C.c_void_p), ("n", C.c_uint32),
                ("reserved", C.c_uint32), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("d_results", C.c_void_p)]


# lzop (la_lzop_block, la_lzop_result, la_lzop_batch)
LZOP_BLOCK_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("src_len", "<u4"), ("dst_len", "<u4"), ("flags", "<u4"),
                             ("sum_c", "<u4"), ("sum_u", "<u4"), ("reserved", "<u4")])
LZOP_RESULT_DTYPE = np.dtype([("status", "<u4"), ("sum_c", "<u4"), ("sum_u", "<u4"), ("out_len", "<u4"), ("consumed", "<u4")])
LA_LZOP_C_ADLER32, LA_LZOP_C_CRC32, LA_LZOP_U_ADLER32, LA_LZOP_U_CRC32 = 1, 2, 4, 8
LA_LZOP_MAX_BLOCK = 64 << 20
(LA_ST_LZOP_BAD_SUM_C, LA_ST_LZOP_INPUT_OVERRUN, LA_ST_LZOP_OUTPUT_OVERRUN, LA_ST_LZOP_LOOKBEHIND, LA_ST_LZOP_NOT_CONSUMED,
 LA_ST_LZOP_SHORT_OUTPUT, LA_ST_LZOP_BAD_SUM_U, LA_ST_LZOP_REFUSED) = 41, 42, 43, 44, 45, 46, 47, 48


class _LzopBatchC(C.Structure):     # la_lzop_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("d_blocks", C.c_void_p), ("n", C.c_uint32),
                ("reserved", C.c_uint32), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("d_results", C.c_void_p)]


# uu (la_uu_state, la_uu_result, la_uu_batch)
UU_RESULT_DTYPE = np.dtype([("status", "<u4"), ("state", "<u4"), ("decoded", "<u4"), ("n_headers", "<u4"), ("out_len", "<u8"),
                            ("consumed", "<u8"), ("stop_off", "<u8"), ("head_off", "<u8"), ("head_len", "<u4"), ("reserved", "<u4")])
LA_UU_FIND_HEAD, LA_UU_READ_UU, LA_UU_UUEND, LA_UU_READ_BASE64, LA_UU_STOP = 0, 1, 2, 3, 4
LA_UU_MAX_HEAD_LINE, LA_UU_MAX_DATA_LINE, LA_UU_MAX_SRC_BYTES = 131072, 32768, 1 << 31
(LA_ST_UU_IGNORED, LA_ST_UU_BAD_BYTE_HEAD, LA_ST_UU_BAD_BYTE, LA_ST_UU_BAD_LINE, LA_ST_UU_BAD_END, LA_ST_UU_TOO_LONG,
 LA_ST_UU_UNTERMINATED) = 49, 50, 51, 52, 53, 54, 55


class _UuStateC(C.Structure):       # la_uu_state
    _fields_ = [("state", C.c_uint32), ("decoded", C.c_uint32)]


class _UuBatchC(C.Structure):       # la_uu_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("final", C.c_uint32), ("reserved", C.c_uint32),
                ("state_in", _UuStateC), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("d_result", C.c_void_p)]


class _LzcBatchC(C.Structure):      # la_lzc_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("level", C.c_uint32), ("flags", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p)]


LA_LZOPC_BLOCK_BYTES = 65536


class _LzopcBatchC(C.Structure):    # la_lzopc_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("block_size", C.c_uint32), ("lead_bytes", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p)]


class _Bz2StateC(C.Structure):
    _fields_ = [("open", C.c_uint32), ("level", C.c_uint32), ("crc", C.c_uint32), ("stop", C.c_uint32),
                ("start_bit", C.c_uint64), ("total_out", C.c_uint64), ("n_taken", C.c_uint32), ("stop_entry", C.c_uint32),
                ("first_bad", C.c_uint32), ("reserved", C.c_uint32)]


class _Bz2BatchC(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("d_cands", C.c_void_p), ("n", C.c_uint32),
                ("phase", C.c_uint32), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("d_results", C.c_void_p),
                ("state_in", C.POINTER(_Bz2StateC)), ("d_state_out", C.c_void_p), ("options", C.c_uint32),
                ("slot_level", C.c_uint32), ("n_emit", C.c_uint32), ("reserved", C.c_uint32)]


class _GzcFramingC(C.Union):     # the header's anonymous union: `reserved` is the field's earlier name
    _fields_ = [("framing", C.c_uint32), ("reserved", C.c_uint32)]


class _GzcBatchC(C.Structure):
    _anonymous_ = ("_framing",)
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("chunk_bytes", C.c_uint32), ("mtime", C.c_uint32),
        ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p),
        ("options", C.c_uint32), ("_framing", _GzcFramingC),
    ]


LA_GZC_FIXED, LA_GZC_DYNAMIC, LA_GZC_STORED = 0, 1, 2
LA_ZIPC_LAST, LA_ZIPC_STORE = 1, 2
LA_ERR_ARG = -3
ZIPC_SEG_DTYPE = np.dtype([("src_off", "<u8"), ("src_len", "<u4"), ("crc_seed", "<u4"), ("gap_before", "<u4"),
                           ("gap_after", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
ZIPC_RESULT_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u4"), ("crc32", "<u4")])
assert ZIPC_SEG_DTYPE.itemsize == 32 and ZIPC_RESULT_DTYPE.itemsize == 16


class _ZipcBatchC(C.Structure):
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("d_segs", C.c_void_p), ("n_segs", C.c_uint32), ("chunk_bytes", C.c_uint32),
        ("options", C.c_uint32), ("reserved", C.c_uint32),
        ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_results", C.c_void_p), ("d_out_bytes", C.c_void_p),
    ]

LA_GZC_FRAME_MEMBERS, LA_GZC_FRAME_STREAM = 0, 1


class _GzHistC(C.Union):        # the header's anonymous union: `reserved` is the field's earlier name
    _fields_ = [("hist_len", C.c_uint32), ("reserved", C.c_uint32)]


class _GzBatchC(C.Structure):
    _anonymous_ = ("_hist",)
    _fields_ = [
        ("d_src", C.c_void_p), ("src_bytes", C.c_uint64),
        ("d_members", C.c_void_p), ("n_members", C.c_uint32),
        ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64),
        ("d_results", C.c_void_p), ("d_summary", C.c_void_p),
        ("options", C.c_uint32), ("_hist", _GzHistC),
    ]


class _Lz4IndexC(C.Structure):
    _fields_ = [
        ("blocks", C.c_void_p), ("n_blocks", C.c_uint32), ("cap_blocks", C.c_uint32),
        ("frames", C.c_void_p), ("n_frames", C.c_uint32), ("cap_frames", C.c_uint32),
        ("end_kind", C.c_int), ("consumed", C.c_uint64), ("max_out", C.c_uint64),
    ]


_gpu = None
_host = None


def gpu_lib():
    """libla_gpu.so (HIP kernels + C shim).  Raises when it has not been built."""
    global _gpu
    if _gpu is None:
        if not os.path.exists(GPU_LIB_PATH):
            raise NativeLibraryMissing(
                "%s not found: build it with `make -C libarchive_amd/csrc` (hipcc, gfx950); "
                "there is no CPU fallback" % GPU_LIB_PATH)
        # This harness shares device buffers with PyTorch, and the PyTorch wheel carries its own HIP runtime: it has to
        # be the one already loaded when libla_gpu.so resolves libamdhip64, or the process ends up with two runtimes and
        # la_gpu_open() sees no device (found with `python __graft_entry__.py smoke`, where build() loaded this library
        # before smoke() imported torch).  A C caller (la_cat, the filters inside libarchive) links the system runtime
        # and never meets torch.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(GPU_LIB_PATH)
        lib.la_gpu_abi_version.restype = C.c_int
        lib.la_gpu_device_count.restype = C.c_int
        lib.la_gpu_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.la_gpu_close.argtypes = [C.c_void_p]
        lib.la_gpu_close.restype = None
        lib.la_gpu_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.la_gpu_sync.argtypes = [C.c_void_p]
        lib.la_gpu_last_error.argtypes = [C.c_void_p]
        lib.la_gpu_last_error.restype = C.c_char_p
        lib.la_gpu_reserve.argtypes = [C.c_void_p, C.c_uint64]
        lib.la_gpu_timer_start.argtypes = [C.c_void_p]
        lib.la_gpu_timer_stop.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        lib.la_gpu_profile_enable.argtypes = [C.c_void_p, C.c_int]
        lib.la_gpu_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]
        lib.la_gpu_xxh32_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.la_gpu_crc32_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.la_gpu_lz4_workspace_bytes.argtypes = [C.c_uint32, C.c_uint64]
        lib.la_gpu_lz4_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_lz4_decode.argtypes = [C.c_void_p, C.POINTER(_Lz4BatchC)]
        lib.la_gpu_lz4_debug_deps.argtypes = [C.c_void_p, C.POINTER(_Lz4BatchC), C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_uint32]
        lib.la_gpu_lz4_debug_literal_plan.argtypes = [C.c_void_p, C.POINTER(_Lz4BatchC), C.c_uint32, C.c_void_p, C.c_uint32]
        lib.la_gpu_lz4_compress.argtypes = [C.c_void_p, C.POINTER(_Lz4cBatchC)]
        lib.la_gpu_gzip_compress.argtypes = [C.c_void_p, C.POINTER(_GzcBatchC)]
        lib.la_gpu_gzip_compress_bound.restype = C.c_uint64
        lib.la_gpu_gzip_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_gzip_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_gzip_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_lz4_compress_bound.restype = C.c_uint64
        lib.la_gpu_lz4_compress_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        lib.la_gpu_lz4_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_lz4_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        lib.la_gpu_gzip_decode.argtypes = [C.c_void_p, C.POINTER(_GzBatchC)]
        lib.la_gpu_zip_compress.argtypes = [C.c_void_p, C.POINTER(_ZipcBatchC)]
        lib.la_gpu_zip_compress_bound.restype = C.c_uint64
        lib.la_gpu_zip_compress_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
        lib.la_gpu_zip_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_zip_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        lib.la_gpu_zstd_compress.argtypes = [C.c_void_p, C.POINTER(_ZstdcBatchC)]
        lib.la_gpu_bzip2_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.la_gpu_bzip2_decode.argtypes = [C.c_void_p, C.POINTER(_Bz2BatchC)]
        lib.la_gpu_bzip2_max_blocks.restype = C.c_uint32
        lib.la_gpu_bzip2_max_blocks.argtypes = [C.c_uint32]
        lib.la_gpu_bzip2_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_bzip2_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.la_gpu_bzip2_compress.argtypes = [C.c_void_p, C.POINTER(_Bz2cBatchC)]
        lib.la_gpu_xz_decode.argtypes = [C.c_void_p, C.POINTER(_XzBatchC)]
        lib.la_gpu_xz_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_xz_workspace_bytes.argtypes = [C.c_uint32]
        lib.la_gpu_xz_compress.argtypes = [C.c_void_p, C.POINTER(_XzcBatchC)]
        lib.la_gpu_lzip_compress.argtypes = [C.c_void_p, C.POINTER(_LzcBatchC)]
        lib.la_gpu_lzip_compress_member_bytes.restype = C.c_uint64
        lib.la_gpu_lzip_compress_member_bytes.argtypes = [C.c_uint32]
        lib.la_gpu_lzip_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_lzip_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_lzip_compress_bound.restype = C.c_uint64
        lib.la_gpu_lzip_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_lzip_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.la_gpu_lzip_decode.argtypes = [C.c_void_p, C.POINTER(_LzipBatchC)]
        lib.la_gpu_lzip_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_lzip_workspace_bytes.argtypes = [C.c_uint32]
        lib.la_gpu_adler32_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.la_gpu_lzop_decode.argtypes = [C.c_void_p, C.POINTER(_LzopBatchC)]
        lib.la_gpu_lzop_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_lzop_workspace_bytes.argtypes = [C.c_uint32]
        lib.la_gpu_lzop_compress.argtypes = [C.c_void_p, C.POINTER(_LzopcBatchC)]
        lib.la_gpu_uu_decode.argtypes = [C.c_void_p, C.POINTER(_UuBatchC)]
        lib.la_gpu_uu_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_uu_workspace_bytes.argtypes = [C.c_uint64]
        lib.la_gpu_lzop_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_lzop_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_lzop_compress_bound.restype = C.c_uint64
        lib.la_gpu_lzop_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_xz_compress_block_bytes.restype = C.c_uint64
        lib.la_gpu_xz_compress_block_bytes.argtypes = [C.c_uint32]
        lib.la_gpu_xz_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_xz_compress_workspace_bytes.argtypes = [C.c_uint64]
        lib.la_gpu_xz_compress_bound.restype = C.c_uint64
        lib.la_gpu_xz_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_bzip2_compress_block_bytes.restype = C.c_uint32
        lib.la_gpu_bzip2_compress_block_bytes.argtypes = [C.c_uint32]
        lib.la_gpu_bzip2_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_bzip2_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_bzip2_compress_sort_rounds.restype = C.c_uint32
        lib.la_gpu_bzip2_compress_sort_rounds.argtypes = [C.c_void_p]
        lib.la_gpu_bzip2_compress_bound.restype = C.c_uint64
        lib.la_gpu_bzip2_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_zstd_compress_bound.restype = C.c_uint64
        lib.la_gpu_zstd_compress_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        lib.la_gpu_zstd_compress_workspace_bytes.restype = C.c_uint64
        lib.la_gpu_zstd_compress_workspace_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        _gpu = lib
    return _gpu


def host_lib():
    """libla_host.so (plain-C walkers / read core / filters)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise NativeLibraryMissing(
                "%s not found: build it with `make -C libarchive_amd/host`" % HOST_LIB_PATH)
        lib = C.CDLL(HOST_LIB_PATH)
        lib.la_lz4_index_build.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(_Lz4IndexC)]
        lib.la_lz4_index_free.argtypes = [C.POINTER(_Lz4IndexC)]
        lib.la_lz4_index_free.restype = None
        lib.la_lz4_bid_bytes.argtypes = [C.c_char_p, C.c_size_t]
        lib.la_status_message.argtypes = [C.c_uint32]
        lib.la_status_message.restype = C.c_char_p
        lib.la_end_message.argtypes = [C.c_int, C.c_int]
        lib.la_end_message.restype = C.c_char_p
        _host = lib
    return _host


def status_message(st: int) -> str:
    return host_lib().la_status_message(int(st)).decode()


def end_message(kind: int, is_gzip: bool = False) -> str:
    return host_lib().la_end_message(int(kind), 1 if is_gzip else 0).decode()


class Lz4Index:
    """Block / frame job tables of a .lz4 image (host walker, la_lz4_index_build)."""

    def __init__(self, blocks, frames, end_kind, consumed, max_out):
        self.blocks = blocks
        self.frames = frames
        self.end_kind = end_kind
        self.consumed = consumed
        self.max_out = max_out


def lz4_index(image, at_eof: bool = True) -> Lz4Index:
    """Walk a compressed image (bytes or uint8 ndarray) on the host."""
    if isinstance(image, (bytes, bytearray, memoryview)):
        image = np.frombuffer(bytes(image), dtype=np.uint8)
    image = np.ascontiguousarray(image, dtype=np.uint8)
    c = _Lz4IndexC()
    rc = host_lib().la_lz4_index_build(image.ctypes.data, image.size, 1 if at_eof else 0, C.byref(c))
    if rc != 0:
        raise MemoryError("la_lz4_index_build")
    try:
        blocks = np.empty(c.n_blocks, dtype=LZ4_BLOCK_DTYPE)
        frames = np.empty(c.n_frames, dtype=LZ4_FRAME_DTYPE)
        if c.n_blocks:
            C.memmove(blocks.ctypes.data, c.blocks, blocks.nbytes)
        if c.n_frames:
            C.memmove(frames.ctypes.data, c.frames, frames.nbytes)
        return Lz4Index(blocks, frames, c.end_kind, c.consumed, c.max_out)
    finally:
        host_lib().la_lz4_index_free(C.byref(c))


GZ_HEADER_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("mtime", "<u4"), ("name_off", "<u4"), ("bgzf_size", "<u4")])


class _GzIndexC(C.Structure):
    _fields_ = [("members", C.c_void_p), ("headers", C.c_void_p), ("n", C.c_uint32), ("cap", C.c_uint32),
                ("end_kind", C.c_int), ("consumed", C.c_uint64), ("max_out", C.c_uint64), ("speculative", C.c_int)]


class GzIndex:
    """Member table of a .gz image (host walker, la_gz_index_build)."""

    def __init__(self, members, headers, end_kind, consumed, max_out, speculative):
        self.members, self.headers = members, headers
        self.end_kind, self.consumed, self.max_out, self.speculative = end_kind, consumed, max_out, speculative


def gz_index(image, at_eof: bool = True) -> GzIndex:
    if isinstance(image, (bytes, bytearray, memoryview)):
        image = np.frombuffer(bytes(image), dtype=np.uint8)
    image = np.ascontiguousarray(image, dtype=np.uint8)
    lib = host_lib()
    lib.la_gz_index_build.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(_GzIndexC)]
    lib.la_gz_index_free.argtypes = [C.POINTER(_GzIndexC)]
    lib.la_gz_index_free.restype = None
    c = _GzIndexC()
    if lib.la_gz_index_build(image.ctypes.data, image.size, 1 if at_eof else 0, C.byref(c)) != 0:
        raise MemoryError("la_gz_index_build")
    try:
        mem = np.empty(c.n, dtype=GZ_MEMBER_DTYPE)
        hdr = np.empty(c.n, dtype=GZ_HEADER_DTYPE)
        if c.n:
            C.memmove(mem.ctypes.data, c.members, mem.nbytes)
            C.memmove(hdr.ctypes.data, c.headers, hdr.nbytes)
        return GzIndex(mem, hdr, c.end_kind, c.consumed, c.max_out, c.speculative)
    finally:
        lib.la_gz_index_free(C.byref(c))


class _GzPiecesC(C.Structure):
    _fields_ = [("pieces", C.c_void_p), ("n", C.c_uint32), ("cap", C.c_uint32), ("end_kind", C.c_int),
                ("last_open", C.c_int), ("consumed", C.c_uint64), ("max_out", C.c_uint64)]


class GzPieces:
    """Piece table of one member body (host walker, la_gz_pieces_build): `members` has the layout of GzIndex.members."""

    def __init__(self, members, end_kind, last_open, consumed, max_out):
        self.members, self.end_kind, self.last_open = members, end_kind, bool(last_open)
        self.consumed, self.max_out = consumed, max_out


def gz_pieces(image, start=0, at_eof=True, first_skip=0, min_cap=0, out_budget=0, span_limit=0xFFFFFFFF) -> GzPieces:
    """Cut image[start:] -- `start` on a byte-aligned deflate block boundary -- at its flush markers."""
    if isinstance(image, (bytes, bytearray, memoryview)):
        image = np.frombuffer(bytes(image), dtype=np.uint8)
    image = np.ascontiguousarray(image, dtype=np.uint8)
    lib = host_lib()
    lib.la_gz_pieces_build.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32,
                                       C.c_uint64, C.c_uint64, C.POINTER(_GzPiecesC)]
    lib.la_gz_pieces_free.argtypes = [C.POINTER(_GzPiecesC)]
    lib.la_gz_pieces_free.restype = None
    c = _GzPiecesC()
    if lib.la_gz_pieces_build(image.ctypes.data, image.size, start, 1 if at_eof else 0, first_skip, min_cap,
                              out_budget, span_limit, C.byref(c)) != 0:
        raise MemoryError("la_gz_pieces_build")
    try:
        mem = np.empty(c.n, dtype=GZ_MEMBER_DTYPE)
        if c.n:
            C.memmove(mem.ctypes.data, c.pieces, mem.nbytes)
        return GzPieces(mem, c.end_kind, c.last_open, c.consumed, c.max_out)
    finally:
        lib.la_gz_pieces_free(C.byref(c))


class GpuContext:
    """la_gpu_ctx: one HIP stream + workspace on one device."""

    def __init__(self, device: int = 0, stream=None):
        lib = gpu_lib()
        h = C.c_void_p()
        rc = lib.la_gpu_open(device, C.byref(h))
        if rc != LA_OK:
            raise RuntimeError("la_gpu_open(%d) failed with %d: no usable gfx950 device "
                               "(there is no CPU fallback)" % (device, rc))
        self._h = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def _check(self, rc, what):
        if rc != LA_OK:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, gpu_lib().la_gpu_last_error(self._h).decode()))

    def set_stream(self, cuda_stream_handle):
        self._check(gpu_lib().la_gpu_set_stream(self._h, C.c_void_p(cuda_stream_handle)), "la_gpu_set_stream")

    def reserve(self, nbytes):
        self._check(gpu_lib().la_gpu_reserve(self._h, int(nbytes)), "la_gpu_reserve")

    def sync(self):
        self._check(gpu_lib().la_gpu_sync(self._h), "la_gpu_sync")

    def timer_start(self):
        self._check(gpu_lib().la_gpu_timer_start(self._h), "la_gpu_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(gpu_lib().la_gpu_timer_stop(self._h, C.byref(ms)), "la_gpu_timer_stop")
        return ms.value

    def profile_enable(self, on=True):
        self._check(gpu_lib().la_gpu_profile_enable(self._h, 1 if on else 0), "la_gpu_profile_enable")

    def profile_read(self):
        """{phase name: ms} of the most recent batch call (synchronises)."""
        ms = (C.c_float * 12)()
        names = (C.c_char_p * 12)()
        n = gpu_lib().la_gpu_profile_read(self._h, ms, names, 12)
        if n < 0:
            self._check(n, "la_gpu_profile_read")
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def xxh32_many(self, d_base_ptr, d_jobs_ptr, n, d_out_ptr):
        self._check(gpu_lib().la_gpu_xxh32_many(self._h, d_base_ptr, d_jobs_ptr, n, d_out_ptr), "la_gpu_xxh32_many")

    def crc32_many(self, d_base_ptr, d_jobs_ptr, n, d_out_ptr):
        self._check(gpu_lib().la_gpu_crc32_many(self._h, d_base_ptr, d_jobs_ptr, n, d_out_ptr), "la_gpu_crc32_many")

    def lz4_decode(self, batch: _Lz4BatchC):
        self._check(gpu_lib().la_gpu_lz4_decode(self._h, C.byref(batch)), "la_gpu_lz4_decode")

    def lz4_debug_deps(self, batch: _Lz4BatchC, block: int, cap: int = 4096):
        """(table entries as uint64, dependency words as uint32) of one block of the decode that just ran with `batch`;
        cut to the block's sequence count, at most cap (la_gpu_lz4_debug_deps)."""
        seq, deps = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        n = gpu_lib().la_gpu_lz4_debug_deps(self._h, C.byref(batch), block, seq.ctypes.data, deps.ctypes.data, cap)
        if n < 0:
            self._check(n, "la_gpu_lz4_debug_deps")
        return seq[:min(n, cap)], deps[:min(n, cap)]

    def lz4_debug_literal_plan(self, batch: _Lz4BatchC, block: int, cap: int = 2049):
        """The literal plan of one window block of the decode that just ran with `batch` (la_gpu_lz4_debug_literal_plan):
        per 32-byte payload chunk the first sequence with literals in or behind it (0xFFFF: none), then the number of
        chunks that hold literals; uint16, empty for a block without a plan."""
        plan = np.zeros(cap, dtype=np.uint16)
        n = gpu_lib().la_gpu_lz4_debug_literal_plan(self._h, C.byref(batch), block, plan.ctypes.data, cap)
        if n < 0:
            self._check(n, "la_gpu_lz4_debug_literal_plan")
        return plan[:min(n, cap)]

    def lz4_compress(self, batch: _Lz4cBatchC):
        self._check(gpu_lib().la_gpu_lz4_compress(self._h, C.byref(batch)), "la_gpu_lz4_compress")

    def zstd_compress(self, batch: _ZstdcBatchC):
        self._check(gpu_lib().la_gpu_zstd_compress(self._h, C.byref(batch)), "la_gpu_zstd_compress")

    def bzip2_compress(self, batch: _Bz2cBatchC):
        self._check(gpu_lib().la_gpu_bzip2_compress(self._h, C.byref(batch)), "la_gpu_bzip2_compress")

    def gzip_compress(self, batch: _GzcBatchC):
        self._check(gpu_lib().la_gpu_gzip_compress(self._h, C.byref(batch)), "la_gpu_gzip_compress")

    def zip_compress(self, batch: _ZipcBatchC) -> int:
        """la_gpu_zip_compress; returns LA_OK or LA_ERR_ARG (the segment table is checked on the device), raises otherwise"""
        rc = gpu_lib().la_gpu_zip_compress(self._h, C.byref(batch))
        if rc != LA_ERR_ARG:
            self._check(rc, "la_gpu_zip_compress")
        return rc

    def bzip2_scan(self, d_src_ptr, src_bytes, d_cands_ptr, cand_cap, d_count_ptr):
        self._check(gpu_lib().la_gpu_bzip2_scan(self._h, d_src_ptr, src_bytes, d_cands_ptr, cand_cap, d_count_ptr), "la_gpu_bzip2_scan")

    def bzip2_decode(self, batch: _Bz2BatchC):
        self._check(gpu_lib().la_gpu_bzip2_decode(self._h, C.byref(batch)), "la_gpu_bzip2_decode")

    def xz_decode(self, batch: _XzBatchC):
        self._check(gpu_lib().la_gpu_xz_decode(self._h, C.byref(batch)), "la_gpu_xz_decode")

    def xz_compress(self, batch: _XzcBatchC):
        self._check(gpu_lib().la_gpu_xz_compress(self._h, C.byref(batch)), "la_gpu_xz_compress")

    def lzip_scan(self, d_src_ptr, src_bytes, d_offs_ptr, cap, d_count_ptr):
        self._check(gpu_lib().la_gpu_lzip_scan(self._h, d_src_ptr, src_bytes, d_offs_ptr, cap, d_count_ptr), "la_gpu_lzip_scan")

    def lzip_decode(self, batch: _LzipBatchC):
        self._check(gpu_lib().la_gpu_lzip_decode(self._h, C.byref(batch)), "la_gpu_lzip_decode")

    def adler32_many(self, d_base_ptr, d_jobs_ptr, n, d_out_ptr):
        self._check(gpu_lib().la_gpu_adler32_many(self._h, d_base_ptr, d_jobs_ptr, n, d_out_ptr), "la_gpu_adler32_many")

    def lzop_decode(self, batch: _LzopBatchC):
        self._check(gpu_lib().la_gpu_lzop_decode(self._h, C.byref(batch)), "la_gpu_lzop_decode")

    def uu_decode(self, batch: _UuBatchC):
        self._check(gpu_lib().la_gpu_uu_decode(self._h, C.byref(batch)), "la_gpu_uu_decode")

    def lzop_compress(self, batch: _LzopcBatchC):
        self._check(gpu_lib().la_gpu_lzop_compress(self._h, C.byref(batch)), "la_gpu_lzop_compress")

    def lzip_compress(self, batch: _LzcBatchC):
        self._check(gpu_lib().la_gpu_lzip_compress(self._h, C.byref(batch)), "la_gpu_lzip_compress")

    def gzip_decode(self, batch: _GzBatchC):
        self._check(gpu_lib().la_gpu_gzip_decode(self._h, C.byref(batch)), "la_gpu_gzip_decode")

    def close(self):
        if getattr(self, "_h", None):
            gpu_lib().la_gpu_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
