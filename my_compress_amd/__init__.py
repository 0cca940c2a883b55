"""my_compress_amd — MI355X-native LZ77 + Huffman compressor (FCX7 byte stream).

Python mirror of the reference's compress interface over the C ABI in
include/fcx.h (lib/libfcx.so, hand-written HIP kernels for gfx950):

    my_compress_file_lz77(block) -> payload      # my_compress.cpp:2115
    my_decompress_file_lz77(payload) -> block    # my_compress.cpp:2255
    compress(data, block_bytes) -> FCX7 file     # main() compress loop, :4073-4136
    decompress(blob) -> data                     # main() decompress loop, :4137-4204
    Context(...).compress_shard(d_in, n, d_out, cap, stream)   # device-resident batch

The compress path runs only on the GPU: a missing extension or device raises
(FcxError / ImportError); there is no CPU fallback.
"""
import ctypes
import os
import struct

__all__ = [
    "FcxError", "lib", "lib_path", "Context", "my_compress_file_lz77", "my_decompress_file_lz77",
    "compress", "decompress", "verify", "repair", "decompress_repaired", "parse_repair", "RepairEntry", "digest", "parse_digest", "check", "find", "count_lines", "decompress_lines", "line_numbers", "find_lines", "grep", "grep_ranges", "PatternSet", "find_any", "grep_any", "grep_any_ranges", "grep_context", "grep_context_blocks", "Regex", "grep_regex", "grep_regex_blocks", "Cut", "cut", "cut_size", "shard_bound", "write_header", "BLOCK_BYTES", "HEADER_BYTES",
]

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
BLOCK_BYTES = 1 << 20   # BLOCK_BYTES, my_compress.cpp:113
HEADER_BYTES = 10       # stCmpFileHead, my_compress.cpp:101-109

_lib = None


class FcxError(RuntimeError):
    pass


def lib_path() -> str:
    # FCX_LIB: alternative in-tree build for A/B experiments (tools/); default lib/libfcx.so
    return os.environ.get("FCX_LIB") or os.path.join(PKG_DIR, "lib", "libfcx.so")


def lib():
    """Load lib/libfcx.so (built by __graft_entry__.build()); raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(path)
    c_u8p = ctypes.c_void_p
    L.fcx_compress_block.argtypes = [ctypes.c_void_p, ctypes.c_uint32, c_u8p]
    L.fcx_compress_block.restype = ctypes.c_uint32
    L.fcx_decompress_block.argtypes = [c_u8p, ctypes.c_uint32, c_u8p, ctypes.c_uint64]
    L.fcx_decompress_block.restype = ctypes.c_int64
    L.fcx_write_header.argtypes = [c_u8p, ctypes.c_uint64, ctypes.c_uint64]
    L.fcx_parse_header.argtypes = [c_u8p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint16),
                                   ctypes.c_char_p]
    L.fcx_shard_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.fcx_shard_bound.restype = ctypes.c_uint64
    L.fcx_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64]
    L.fcx_ctx_destroy.argtypes = [ctypes.c_void_p]
    L.fcx_ctx_destroy.restype = None
    L.fcx_compress_shard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    L.fcx_ctx_device_out_len.argtypes = [ctypes.c_void_p]
    L.fcx_ctx_device_out_len.restype = ctypes.c_void_p
    L.fcx_ctx_read_out_len.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    L.fcx_compress_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64,
                                    ctypes.POINTER(ctypes.c_uint64)]
    L.fcx_ctx_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.fcx_ctx_set_match_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.fcx_ctx_stage_count.argtypes = [ctypes.c_void_p]
    L.fcx_ctx_stage.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                ctypes.POINTER(ctypes.c_float)]
    L.fcx_ctx_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint64)] * 5
    L.fcx_ctx_match_kernel.argtypes = [ctypes.c_void_p]
    L.fcx_ctx_match_kernel.restype = ctypes.c_int
    if hasattr(L, "fcx_ctx_route_stats"):   # (absent from an older FCX_LIB build used for A/B timing)
        L.fcx_ctx_route_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.fcx_compress_stream.argtypes = [ctypes.c_void_p, READ_FN, WRITE_FN, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint64)]
    L.fcx_decompress_stream.argtypes = [ctypes.c_void_p, READ_FN, WRITE_FN, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64),
                                        ctypes.POINTER(ctypes.c_uint64)]
    L.fcx_dctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    L.fcx_dctx_destroy.argtypes = [ctypes.c_void_p]
    L.fcx_dctx_destroy.restype = None
    L.fcx_decompress_shard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.c_void_p]
    L.fcx_decompress_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64,
                                      ctypes.POINTER(ctypes.c_uint64)]
    L.fcx_dctx_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.fcx_dctx_stage_count.argtypes = [ctypes.c_void_p]
    L.fcx_dctx_stage.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                 ctypes.POINTER(ctypes.c_float)]
    L.fcx_dctx_symbol_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.fcx_lz78_compress_shard.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    L.fcx_lz78_compress_host.argtypes = [c_u8p, ctypes.c_uint64, ctypes.c_uint32, c_u8p, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_uint64)]
    L.fcx_lz78_compress_block.argtypes = [ctypes.c_void_p, ctypes.c_uint32, c_u8p]
    L.fcx_lz78_compress_block.restype = ctypes.c_uint32
    L.fcx_lz78_release.argtypes = []
    L.fcx_lz78_decompress_block.argtypes = [c_u8p, ctypes.c_uint32, c_u8p, ctypes.c_uint64]
    L.fcx_lz78_decompress_block.restype = ctypes.c_int64
    L.fcx_lz78_decompress_host.argtypes = [c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "fcx_lz78_decompress_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        L.fcx_lz78_decompress_shard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.c_void_p]
        L.fcx_lz78_decode_batch_records.argtypes = []
        L.fcx_lz78_decode_batch_records.restype = ctypes.c_uint32
    P64 = ctypes.POINTER(ctypes.c_uint64)
    if hasattr(L, "fcx_index_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        L.fcx_index_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p, P64, ctypes.c_void_p]
        L.fcx_decompress_range_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, P64, ctypes.c_void_p]
        L.fcx_decompress_range_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                c_u8p, ctypes.c_uint64, P64]
        L.fcx_decompress_range_stream.argtypes = [ctypes.c_void_p, READ_FN, WRITE_FN, ctypes.c_void_p, ctypes.c_uint64,
                                                  ctypes.c_uint64, ctypes.c_uint64, P64]
        L.fcx_dctx_range_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
    if hasattr(L, "fcx_verify_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        L.fcx_verify_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, P64,
                                       ctypes.c_void_p]
        L.fcx_verify_host.argtypes = [ctypes.c_void_p, ctypes.c_char, c_u8p, ctypes.c_uint64, ctypes.c_uint32, c_u8p,
                                      ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, P64]
        L.fcx_verify_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, READ_FN, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_uint64, VERIFY_FN, ctypes.c_void_p, P64]
        L.fcx_dctx_set_verify_group.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.fcx_dctx_verify_groups.argtypes = [ctypes.c_void_p]
    if hasattr(L, "fcx_repair_build_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        P32 = ctypes.POINTER(ctypes.c_uint32)
        L.fcx_repair_build_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint64, P32, P64, P64, ctypes.c_void_p]
        L.fcx_repair_apply_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, P64,
                                             ctypes.c_void_p]
        L.fcx_dctx_repair_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
        L.fcx_repair_build_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, READ_FN, ctypes.c_void_p,
                                              ctypes.c_uint32, ctypes.c_uint64, WRITE_FN, ctypes.c_void_p, P64]
        L.fcx_repair_apply_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, READ_FN, ctypes.c_void_p, WRITE_FN,
                                              ctypes.c_void_p, ctypes.c_uint64, P64]
        L.fcx_repair_build_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64, ctypes.c_uint32,
                                            c_u8p, ctypes.c_uint64, P64]
        L.fcx_repair_apply_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64, c_u8p,
                                            ctypes.c_uint64, P64]
    if hasattr(L, "fcx_digest_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        P32 = ctypes.POINTER(ctypes.c_uint32)
        L.fcx_digest_shard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, P32,
                                       ctypes.c_void_p]
        L.fcx_check_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, P64, ctypes.c_void_p]
        L.fcx_digest_segments.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.c_void_p]
        L.fcx_crc32.argtypes = [ctypes.c_uint32, c_u8p, ctypes.c_uint64]
        L.fcx_crc32.restype = ctypes.c_uint32
        L.fcx_crc32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        L.fcx_crc32_combine.restype = ctypes.c_uint32
        L.fcx_dctx_digest_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
        L.fcx_dctx_set_digest_slice.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.fcx_digest_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint32, WRITE_FN, ctypes.c_void_p, P64]
        L.fcx_check_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, READ_FN, ctypes.c_void_p, READ_FN,
                                       ctypes.c_void_p, ctypes.c_uint64, VERIFY_FN, ctypes.c_void_p, P64]
        L.fcx_digest_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint32, c_u8p, ctypes.c_uint64, P64]
        L.fcx_check_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint64,
                                     VERIFY_FN, ctypes.c_void_p, P64]
    if hasattr(L, "fcx_find_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        L.fcx_find_shard.argtypes = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                     c_u8p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, P64, ctypes.c_void_p]
        L.fcx_find_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, c_u8p, ctypes.c_uint32,
                                      HIT_FN, ctypes.c_void_p, P64]
        L.fcx_find_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_uint32, P64, ctypes.c_uint64, P64]
        L.fcx_dctx_find_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
        L.fcx_dctx_set_find_window.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    if hasattr(L, "fcx_lines_index_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        run = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8]
        index = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fcx_lines_index_shard.argtypes = run + [ctypes.c_void_p, P64, ctypes.c_void_p]
        L.fcx_lines_locate_shard.argtypes = run + index + [ctypes.c_uint64, ctypes.c_uint64, P64, P64, ctypes.c_void_p]
        L.fcx_decompress_lines_shard.argtypes = run + index + [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, P64,
                                                               ctypes.c_void_p]
        L.fcx_lines_of_shard.argtypes = run + [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.fcx_lines_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, P64]
        L.fcx_lines_locate_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8,
                                              ctypes.c_uint64, ctypes.c_uint64, P64, P64]
        L.fcx_lines_of_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, P64,
                                          ctypes.c_uint64, P64]
        L.fcx_lines_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint8, P64]
        L.fcx_decompress_lines_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_uint64,
                                                ctypes.c_uint64, c_u8p, ctypes.c_uint64, P64]
        L.fcx_lines_of_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint8, P64, ctypes.c_uint64, P64]
        L.fcx_dctx_lines_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
    if hasattr(L, "fcx_grep_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        run = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
        L.fcx_grep_shard.argtypes = run + [ctypes.c_uint8, c_u8p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, P64,
                                           ctypes.c_void_p]
        L.fcx_decompress_ranges_shard.argtypes = run + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                        ctypes.c_void_p, ctypes.c_uint64, P64, ctypes.c_void_p]
        L.fcx_dctx_ranges_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
        L.fcx_dctx_grep_scratch.argtypes = [ctypes.c_void_p, P64]
        L.fcx_grep_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint8, c_u8p, ctypes.c_uint32, c_u8p, ctypes.c_uint64,
                                    P64, P64]
        L.fcx_decompress_ranges_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, P64, P64, ctypes.c_uint64, c_u8p, ctypes.c_uint64,
                                                 P64]
        L.fcx_grep_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, c_u8p, ctypes.c_uint32,
                                      RANGE_FN, ctypes.c_void_p, P64]
        L.fcx_decompress_ranges_stream.argtypes = [ctypes.c_void_p, READ_FN, WRITE_FN, ctypes.c_void_p, ctypes.c_uint64, P64, P64,
                                                   ctypes.c_uint64, P64]
    if hasattr(L, "fcx_pattern_set_create"):   # (absent from an older FCX_LIB build used for A/B timing)
        run = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
        P32 = ctypes.POINTER(ctypes.c_uint32)
        L.fcx_pattern_set_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), c_u8p, P32, ctypes.c_uint32, ctypes.c_uint32]
        L.fcx_pattern_set_destroy.argtypes = [ctypes.c_void_p]
        L.fcx_pattern_set_destroy.restype = None
        L.fcx_pattern_set_info.argtypes = [ctypes.c_void_p, P32, P32, P32, P32]
        L.fcx_find_set_shard.argtypes = run + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, P64, P64, ctypes.c_void_p]
        L.fcx_find_set_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, HIT_FN,
                                          ctypes.c_void_p, P64, P64]
        L.fcx_find_set_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_void_p, P64, ctypes.c_uint64, P64, P64]
        L.fcx_grep_set_shard.argtypes = run + [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, P64,
                                               P64, ctypes.c_void_p]
        L.fcx_grep_set_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_void_p,
                                          RANGE_FN, ctypes.c_void_p, P64, P64]
        L.fcx_grep_set_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_void_p, c_u8p, ctypes.c_uint64,
                                        P64, P64, P64]
        L.fcx_dctx_set_scan_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
    if hasattr(L, "fcx_grep_blocks_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        run = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
        L.fcx_grep_blocks_shard.argtypes = run + [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_uint64, P64, P64, ctypes.c_void_p]
        L.fcx_grep_blocks_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_void_p,
                                             ctypes.c_void_p, BLOCK_FN, ctypes.c_void_p, P64, P64]
        L.fcx_grep_blocks_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p,
                                           c_u8p, ctypes.c_uint64, P64, P64, P64]
    if hasattr(L, "fcx_grep_regex_blocks_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        run = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
        P32 = ctypes.POINTER(ctypes.c_uint32)
        L.fcx_regex_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), c_u8p, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint32]
        L.fcx_regex_destroy.argtypes = [ctypes.c_void_p]
        L.fcx_regex_destroy.restype = None
        L.fcx_regex_info.argtypes = [ctypes.c_void_p, P32, P32, P32, ctypes.POINTER(ctypes.c_uint8)]
        L.fcx_grep_regex_blocks_shard.argtypes = run + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_uint64, P64, ctypes.c_void_p]
        L.fcx_grep_regex_blocks_stream.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.c_void_p, BLOCK_FN, ctypes.c_void_p, P64]
        L.fcx_grep_regex_blocks_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, c_u8p,
                                                 ctypes.c_uint64, P64, P64]
        L.fcx_dctx_regex_scan_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
    if hasattr(L, "fcx_cut_shard"):   # (absent from an older FCX_LIB build used for A/B timing)
        run = [ctypes.c_void_p, ctypes.c_char, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
        P32 = ctypes.POINTER(ctypes.c_uint32)
        P8 = ctypes.POINTER(ctypes.c_uint8)
        out = [ctypes.c_void_p, ctypes.c_uint64, P64, P64]
        L.fcx_cut_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint8,
                                     ctypes.c_uint8, ctypes.c_uint32]
        L.fcx_cut_destroy.argtypes = [ctypes.c_void_p]
        L.fcx_cut_destroy.restype = None
        L.fcx_cut_info.argtypes = [ctypes.c_void_p, P32, P8, P8, P32, P32, P32]
        L.fcx_cut_buffer.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p] + out + [ctypes.c_void_p]
        L.fcx_cut_shard.argtypes = run + [ctypes.c_void_p] + out + [ctypes.c_void_p]
        L.fcx_cut_ranges_shard.argtypes = run + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p] + out + [ctypes.c_void_p]
        L.fcx_cut_stream.argtypes = [ctypes.c_void_p, READ_FN, WRITE_FN, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, P64]
        L.fcx_cut_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_void_p, c_u8p, ctypes.c_uint64, P64, P64]
        L.fcx_cut_ranges_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, P64, P64, ctypes.c_uint64, ctypes.c_void_p, c_u8p,
                                          ctypes.c_uint64, P64, P64]
        L.fcx_dctx_cut_stats.argtypes = [ctypes.c_void_p, P64, ctypes.c_int]
        L.fcx_dctx_cut_scratch.argtypes = [ctypes.c_void_p, P64]
    L.fcx_dist_block_range.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, P64, P64]
    L.fcx_dist_block_range.restype = None
    L.fcx_dist_block_range_w.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, P64, P64]
    L.fcx_dist_block_range_w.restype = None
    L.fcx_dist_gather_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
    L.fcx_dist_gather_bound.restype = ctypes.c_uint64
    L.fcx_dist_compress_gather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, P64,
                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, P64, ctypes.c_void_p]
    L.fcx_dist_unique_id.argtypes = [c_u8p]
    L.fcx_dist_init_rank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_int]
    L.fcx_dist_init_local.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.fcx_dist_destroy.argtypes = [ctypes.c_void_p]
    L.fcx_dist_destroy.restype = None
    L.fcx_dist_size.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.fcx_dist_concat.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                  ctypes.c_uint64, P64, ctypes.c_int, ctypes.c_void_p]
    L.fcx_dist_compress_host.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
                                         c_u8p, ctypes.c_uint64, P64]
    L.fcx_dist_transport.argtypes = [ctypes.c_void_p]
    L.fcx_dist_transport.restype = ctypes.c_char_p
    L.fcx_loop_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_uint32]
    L.fcx_loop_destroy.argtypes = [ctypes.c_void_p]
    L.fcx_loop_destroy.restype = None
    L.fcx_dist_init_loop.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int]
    L.fcx_dist_init_loop_local.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
                                           ctypes.c_uint32]
    L.fcx_dist_debug_fail.argtypes = [ctypes.c_void_p, ctypes.c_int]
    if hasattr(L, "fcx_dist_gather_copy_ms"):
        L.fcx_dist_gather_copy_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    L.fcx_last_error.restype = ctypes.c_char_p
    L.fcx_version.restype = ctypes.c_char_p
    _lib = L
    return L


# fcx_read_fn / fcx_write_fn (include/fcx.h)
READ_FN = ctypes.CFUNCTYPE(ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64)
WRITE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64)
# fcx_verify_fn: block, its length in the original, its decoded bytes, the first difference
VERIFY_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32)
VERIFY_SAME = 0xFFFFFFFF   # FCX_VERIFY_SAME
# fcx_hit_fn: the decoded offset of a hit
HIT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64)
FIND_MAX_PATTERN = 256     # FCX_FIND_MAX_PATTERN
# fcx_range_fn: start and end of a selected line
RANGE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64)
BLOCK_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64)


class GrepOpts(ctypes.Structure):
    """fcx_grep_opts"""
    _fields_ = [("flags", ctypes.c_uint32), ("before", ctypes.c_uint32), ("after", ctypes.c_uint32)]


# the repair sidecar (include/fcx.h): one 32-byte entry layout on the device, in the FCXR file and here
REPAIR_RAW, REPAIR_FILL = 0, 1
REPAIR_ENTRY_BYTES, REPAIR_HEADER_BYTES, REPAIR_TRAILER_BYTES = 32, 16, 40
_REPAIR_ENTRY = struct.Struct("<QQIIII")


class RepairEntry(tuple):
    """(block, data_off, from, len, kind, fill) of an fcx_repair_entry"""
    __slots__ = ()
    block = property(lambda s: s[0])
    data_off = property(lambda s: s[1])
    start = property(lambda s: s[2])   # the entry's `from`
    len = property(lambda s: s[3])
    kind = property(lambda s: s[4])
    fill = property(lambda s: s[5])

    def pack(self) -> bytes:
        return _REPAIR_ENTRY.pack(*self)


def unpack_repair_entries(raw: bytes, count: int = None):
    count = len(raw) // REPAIR_ENTRY_BYTES if count is None else count
    return [RepairEntry(_REPAIR_ENTRY.unpack_from(raw, REPAIR_ENTRY_BYTES * i)) for i in range(count)]


def parse_repair(blob: bytes) -> dict:
    """an FCXR file taken apart, for tests: kind, block_bytes, the sections as ([RepairEntry], data) with the
    entries' blocks file-wide and data_off into the section's data, and the trailer (n, records, entries,
    data_bytes).  Checks the layout only (ValueError), not the rules of the reader."""
    if len(blob) < REPAIR_HEADER_BYTES or blob[:4] != b"FCXR":
        raise ValueError("not an FCXR file")
    version, kind, zero, block_bytes, zero2 = struct.unpack_from("<BBHII", blob, 4)
    if version != 1 or zero or zero2:
        raise ValueError("bad FCXR header")
    q, sections, trailer = REPAIR_HEADER_BYTES, [], None
    while trailer is None:
        ne, zero, nd = struct.unpack_from("<IIQ", blob, q)
        if ne == 0xFFFFFFFF:
            trailer = struct.unpack_from("<QQQQ", blob, q + 8)
            q += REPAIR_TRAILER_BYTES
            break
        q += 16
        if q + REPAIR_ENTRY_BYTES * ne + nd > len(blob):
            raise ValueError("truncated FCXR section")
        ents = unpack_repair_entries(blob[q:q + REPAIR_ENTRY_BYTES * ne], ne)
        q += REPAIR_ENTRY_BYTES * ne
        sections.append((ents, blob[q:q + nd]))
        q += nd
    if q != len(blob):
        raise ValueError("bytes behind the FCXR trailer")
    return {"kind": chr(kind), "block_bytes": block_bytes, "sections": sections,
            "trailer": dict(zip(("n", "records", "entries", "data_bytes"), trailer))}


# the content digest (include/fcx.h): the FCXD file
DIGEST_HEADER_BYTES, DIGEST_TRAILER_BYTES, DIGEST_SECTION = 16, 24, 4096


def parse_digest(blob: bytes) -> dict:
    """an FCXD file taken apart, for tests: block_bytes, the sections as lists of CRC-32 values, and the
    trailer (n, blocks, crc32 of the whole original, crc32 of the values).  Checks the layout only
    (ValueError), not the rules of the reader."""
    if len(blob) < DIGEST_HEADER_BYTES or blob[:4] != b"FCXD":
        raise ValueError("not an FCXD file")
    version, zero, zero1, block_bytes, zero2 = struct.unpack_from("<BBHII", blob, 4)
    if version != 1 or zero or zero1 or zero2:
        raise ValueError("bad FCXD header")
    q, sections = DIGEST_HEADER_BYTES, []
    while True:
        if q + 8 > len(blob):
            raise ValueError("truncated FCXD file")
        count, zero = struct.unpack_from("<II", blob, q)
        q += 8
        if count == 0:
            break
        if zero or count > DIGEST_SECTION or q + 4 * count > len(blob):
            raise ValueError("bad FCXD section")
        sections.append(list(struct.unpack_from("<%dI" % count, blob, q)))
        q += 4 * count
    if q + DIGEST_TRAILER_BYTES != len(blob):
        raise ValueError("the FCXD trailer is not the last %d bytes" % DIGEST_TRAILER_BYTES)
    return {"block_bytes": block_bytes, "sections": sections,
            "trailer": dict(zip(("n", "blocks", "crc32", "values_crc32"), struct.unpack_from("<QQII", blob, q)))}


def _stream_fns(src, sink):
    """ctypes callbacks over a binary reader (.readinto) and writer (.write)"""
    def rd(_u, buf, cap):
        mv = (ctypes.c_uint8 * cap).from_address(ctypes.addressof(buf.contents))
        return src.readinto(memoryview(mv).cast("B"))

    def wr(_u, buf, n):
        sink.write(ctypes.string_at(buf, n))
        return 0

    return READ_FN(rd), WRITE_FN(wr)


def _check(rc, what):
    if rc != 0:
        raise FcxError(f"{what} failed ({rc}): {lib().fcx_last_error().decode(errors='replace')}")


def shard_bound(n: int, block_bytes: int = BLOCK_BYTES) -> int:
    return int(lib().fcx_shard_bound(n, block_bytes))


def write_header(total_in: int, nblocks: int) -> bytes:
    buf = ctypes.create_string_buffer(HEADER_BYTES)
    _check(lib().fcx_write_header(buf, total_in, nblocks), "fcx_write_header")
    return buf.raw


class Context:
    """fcx_ctx: device, block size, scratch in HBM for shards up to max_shard_bytes."""

    def __init__(self, device: int = 0, block_bytes: int = BLOCK_BYTES, max_shard_bytes: int = BLOCK_BYTES):
        self._h = ctypes.c_void_p()
        self.block_bytes = block_bytes
        _check(lib().fcx_ctx_create(ctypes.byref(self._h), device, block_bytes, max_shard_bytes), "fcx_ctx_create")

    def close(self):
        if self._h:
            lib().fcx_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compress_shard(self, d_in: int, n: int, d_out: int, cap: int, stream: int = 0, sync: bool = True):
        """device pointers in, [u32 len][payload]... at d_out; returns bytes (sync) or None"""
        out = ctypes.c_uint64(0)
        _check(lib().fcx_compress_shard(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                        ctypes.byref(out) if sync else None, ctypes.c_void_p(stream)),
               "fcx_compress_shard")
        return out.value if sync else None

    def device_out_len_ptr(self) -> int:
        return int(lib().fcx_ctx_device_out_len(self._h))

    def read_out_len(self) -> int:
        """waits for the device; output bytes of the last compress_shard"""
        out = ctypes.c_uint64(0)
        _check(lib().fcx_ctx_read_out_len(self._h, ctypes.byref(out)), "fcx_ctx_read_out_len")
        return out.value

    def compress_host(self, data: bytes) -> bytes:
        cap = shard_bound(len(data), self.block_bytes)
        out = ctypes.create_string_buffer(cap)
        got = ctypes.c_uint64(0)
        _check(lib().fcx_compress_host(self._h, data, len(data), out, cap, ctypes.byref(got)), "fcx_compress_host")
        return out.raw[:got.value]

    def compress_stream(self, src, sink, shard_bytes: int):
        """pipelined stream path: records of src (binary reader) to sink (binary writer);
        returns (total_in, total_out, nblocks)"""
        rd, wr = _stream_fns(src, sink)
        vals = [ctypes.c_uint64() for _ in range(3)]
        _check(lib().fcx_compress_stream(self._h, rd, wr, None, shard_bytes, *[ctypes.byref(v) for v in vals]),
               "fcx_compress_stream")
        return tuple(v.value for v in vals)

    def set_profiling(self, on: bool = True):
        _check(lib().fcx_ctx_set_profiling(self._h, 1 if on else 0), "fcx_ctx_set_profiling")

    def set_match_mode(self, mode: int):
        """testing: 0 auto, 1 bucket search, 2 run table for whole tiles, 3 the general
        kernel, 4 the 4-byte-key kernel, 5 the no-filter kernel, 6 the runs kernel, 7 the sparse
        kernel (same output; fcx.h)"""
        _check(lib().fcx_ctx_set_match_mode(self._h, mode), "fcx_ctx_set_match_mode")

    def stage_times(self):
        """[(stage name, device ms)] of the last profiled compress_shard"""
        res = []
        for i in range(lib().fcx_ctx_stage_count(self._h)):
            name = ctypes.c_char_p()
            ms = ctypes.c_float()
            _check(lib().fcx_ctx_stage(self._h, i, ctypes.byref(name), ctypes.byref(ms)), "fcx_ctx_stage")
            res.append((name.value.decode(), ms.value))
        return res

    def stats(self):
        vals = [ctypes.c_uint64() for _ in range(5)]
        _check(lib().fcx_ctx_stats(self._h, *[ctypes.byref(v) for v in vals]), "fcx_ctx_stats")
        return dict(zip(["tokens", "matches", "lazy_evals", "lazy_tiles", "tiles"], [v.value for v in vals]))

    MATCH_KERNELS = ("k_match", "k_match_k4", "k_match_nf", "k_match_runs", "k_match_sparse", "k_match_uniform")

    def match_kernel(self) -> str:
        """the kernel the last compress_shard call's match stage ran (fcx_ctx_match_kernel; routed:
        the unit given the most tiles)"""
        return self.MATCH_KERNELS[lib().fcx_ctx_match_kernel(self._h)]

    ROUTE_STATS = ("sparse", "runs", "key4", "nofilter", "handed_on", "tiles", "rest", "cold", "uniform")

    def route_stats(self) -> dict:
        """how the last (routed) call's tiles were searched (fcx_ctx_route_stats): tiles per unit
        list, tiles handed on (to the no-filter and runs lists), tiles with bytes, tiles left to the
        units' remainder kernels, whether the call waited for its own counts (a context's first
        call), and the uniform unit's tiles"""
        n = len(self.ROUTE_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_ctx_route_stats(self._h, vals, n), "fcx_ctx_route_stats")
        return dict(zip(self.ROUTE_STATS, [int(v) for v in vals]))


class DContext:
    """fcx_dctx: the GPU decoder (my_decompress_file_lz77 :2255 for whole runs of block records)."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        _check(lib().fcx_dctx_create(ctypes.byref(self._h), device), "fcx_dctx_create")

    def close(self):
        if self._h:
            lib().fcx_dctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decompress_shard(self, d_in: int, in_len: int, nblocks: int, d_out: int, cap: int, stream: int = 0) -> int:
        """device records in, decoded bytes at d_out; returns the decoded byte count"""
        out = ctypes.c_uint64(0)
        _check(lib().fcx_decompress_shard(self._h, ctypes.c_void_p(d_in), in_len, nblocks, ctypes.c_void_p(d_out),
                                          cap, ctypes.byref(out), ctypes.c_void_p(stream)), "fcx_decompress_shard")
        return out.value

    def decompress_lz78_shard(self, d_in: int, in_len: int, nblocks: int, d_out: int, cap: int,
                              stream: int = 0) -> int:
        """FCX8 records on the device in, decoded bytes at d_out; returns the decoded byte count"""
        out = ctypes.c_uint64(0)
        _check(lib().fcx_lz78_decompress_shard(self._h, ctypes.c_void_p(d_in), in_len, nblocks,
                                               ctypes.c_void_p(d_out), cap, ctypes.byref(out),
                                               ctypes.c_void_p(stream)), "fcx_lz78_decompress_shard")
        return out.value

    def decompress_host(self, blob: bytes, cap: int = None) -> bytes:
        """a whole FCX7 or FCX8 file -> the decoded bytes, on the GPU"""
        if cap is None:
            cap = max(16, struct.unpack_from("<I", blob, 4)[0] if len(blob) >= HEADER_BYTES else 0)
        out = ctypes.create_string_buffer(cap)
        got = ctypes.c_uint64(0)
        _check(lib().fcx_decompress_host(self._h, blob, len(blob), out, cap, ctypes.byref(got)),
               "fcx_decompress_host")
        return out.raw[:got.value]

    def decompress_stream(self, src, sink):
        """FCX7 or FCX8 file from src (binary reader) to sink through the GPU decoder;
        returns (header total, decoded bytes, records)"""
        rd, wr = _stream_fns(src, sink)
        t = ctypes.c_uint32()
        o, n = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().fcx_decompress_stream(self._h, rd, wr, None, 0, ctypes.byref(t), ctypes.byref(o), ctypes.byref(n)),
               "fcx_decompress_stream")
        return t.value, o.value, n.value

    # ---- random access (fcx_index_shard / fcx_decompress_range_*): kind is "7" (FCX7) or "8" (FCX8) ----
    def index_shard(self, d_in: int, in_len: int, nblocks: int, kind: str, d_rec_off: int, d_dec_off: int,
                    stream: int = 0) -> int:
        """index of a device-resident run into two device arrays of nblocks + 1 u64 (record offsets,
        decoded offsets); returns the decoded total"""
        total = ctypes.c_uint64(0)
        _check(lib().fcx_index_shard(self._h, kind.encode(), ctypes.c_void_p(d_in), in_len, nblocks,
                                     ctypes.c_void_p(d_rec_off), ctypes.c_void_p(d_dec_off), ctypes.byref(total),
                                     ctypes.c_void_p(stream)), "fcx_index_shard")
        return total.value

    def decompress_range_shard(self, d_in: int, in_len: int, nblocks: int, kind: str, off: int, n: int, d_out: int,
                               cap: int, d_rec_off: int = 0, d_dec_off: int = 0, stream: int = 0) -> int:
        """decoded bytes [off, off + n) of a device-resident run to d_out[0 ..); returns their count
        (less than n at the end of the run).  d_rec_off / d_dec_off: an index_shard index, or both 0
        (the call builds its own)."""
        got = ctypes.c_uint64(0)
        _check(lib().fcx_decompress_range_shard(self._h, kind.encode(), ctypes.c_void_p(d_in), in_len, nblocks,
                                                ctypes.c_void_p(d_rec_off or None), ctypes.c_void_p(d_dec_off or None),
                                                off, n, ctypes.c_void_p(d_out), cap, ctypes.byref(got),
                                                ctypes.c_void_p(stream)), "fcx_decompress_range_shard")
        return got.value

    def decompress_range_host(self, blob: bytes, off: int, n: int) -> bytes:
        """decoded bytes [off, off + n) of a whole FCX7 or FCX8 file, on the GPU"""
        out = ctypes.create_string_buffer(max(n, 1))
        got = ctypes.c_uint64(0)
        _check(lib().fcx_decompress_range_host(self._h, blob, len(blob), off, n, out, n, ctypes.byref(got)),
               "fcx_decompress_range_host")
        return out.raw[:got.value]

    def decompress_range_stream(self, src, sink, off: int, n: int) -> int:
        """decoded bytes [off, off + n) of an FCX7 or FCX8 file from src (binary reader) to sink;
        reads no further than the range needs; returns the bytes written"""
        rd, wr = _stream_fns(src, sink)
        o = ctypes.c_uint64()
        _check(lib().fcx_decompress_range_stream(self._h, rd, wr, None, 0, off, n, ctypes.byref(o)),
               "fcx_decompress_range_stream")
        return o.value

    RANGE_STATS = ("sized", "expanded", "stored", "built_index")

    def range_stats(self) -> dict:
        """counters of the last index / range call (fcx_dctx_range_stats): records the size pass
        sized, records expanded, bytes stored to d_out, 1 if the call built its own index"""
        n = len(self.RANGE_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_range_stats(self._h, vals, n), "fcx_dctx_range_stats")
        return dict(zip(self.RANGE_STATS, [int(v) for v in vals]))

    # ---- round-trip verification (fcx_verify_*): does each record decode back to its block? ----
    VERIFY_STATS = ("blocks", "differ", "first", "size_differs", "bytes", "decoded")

    @classmethod
    def _verify_stats(cls, vals) -> dict:
        d = dict(zip(cls.VERIFY_STATS, [int(v) for v in vals]))
        if d["first"] == 2 ** 64 - 1:
            d["first"] = None
        return d

    def verify_shard(self, d_rec: int, rec_len: int, nblocks: int, kind: str, d_orig: int, n: int, block_bytes: int,
                     d_blocks: int = 0, stream: int = 0) -> dict:
        """device records (no header) against the n device bytes they were compressed from, in blocks
        of block_bytes; d_blocks (2 * nblocks u32 on the device, or 0) receives per record the decoded
        bytes and the first difference (VERIFY_SAME: none).  Returns the stats: blocks, differ, first
        (None: no block differs), size_differs, bytes (of the original in differing blocks), decoded."""
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        _check(lib().fcx_verify_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks,
                                      ctypes.c_void_p(d_orig or None), n, block_bytes, ctypes.c_void_p(d_blocks or None),
                                      vals, ctypes.c_void_p(stream)), "fcx_verify_shard")
        return self._verify_stats(vals)

    def verify_host(self, records: bytes, nblocks: int, kind: str, orig: bytes, block_bytes: int):
        """the same on host bytes; returns (stats, [(decoded bytes, first difference)] per record)"""
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        pairs = (ctypes.c_uint32 * max(2 * nblocks, 1))()
        _check(lib().fcx_verify_host(self._h, kind.encode(), records, len(records), nblocks, orig, len(orig), block_bytes,
                                     pairs, vals), "fcx_verify_host")
        return self._verify_stats(vals), [(int(pairs[2 * k]), int(pairs[2 * k + 1])) for k in range(nblocks)]

    def verify_stream(self, src, orig, block_bytes: int = BLOCK_BYTES, max_in: int = 0):
        """a whole FCX7 or FCX8 file from src against the original from orig (binary readers); returns
        (stats, [(block, its length in the original, decoded bytes, first difference)] of the differing
        blocks).  Original bytes behind the last record come last, as block number stats["blocks"].
        The file round-trips when stats["differ"] == 0 and stats["bytes"] == 0.  max_in (0: unknown): the
        bytes behind the header, which bound the staging buffers."""
        rd, _ = _stream_fns(src, None)
        ro, _ = _stream_fns(orig, None)
        bad = []
        cb = VERIFY_FN(lambda _u, k, blen, dec, fd: bad.append((int(k), int(blen), int(dec), int(fd))))
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        _check(lib().fcx_verify_stream(self._h, rd, None, ro, None, block_bytes, max_in, cb, None, vals), "fcx_verify_stream")
        return self._verify_stats(vals), bad

    def set_verify_group(self, nbytes: int):
        """testing: bound of a group's decoded bytes in later verify calls (0: the default, 256 MiB)"""
        _check(lib().fcx_dctx_set_verify_group(self._h, nbytes), "fcx_dctx_set_verify_group")

    def verify_groups(self) -> int:
        """groups the last verify_shard call decoded"""
        return int(lib().fcx_dctx_verify_groups(self._h))

    # ---- the repair sidecar (fcx_repair_*): what restores the blocks that do not come back ----
    REPAIR_STATS = ("entries", "fills", "data_bytes", "groups_direct", "groups_staged")

    def repair_build_shard(self, d_rec: int, rec_len: int, nblocks: int, kind: str, d_orig: int, n: int, block_bytes: int,
                           d_entries: int = 0, d_data: int = 0, data_cap: int = 0, stream: int = 0, check: bool = True):
        """the repair of device records against the n device bytes they were compressed from: the entries
        (32 bytes each, block order) to d_entries (nblocks slots, or 0), the RAW bytes to d_data.  Returns
        (rc, entries, data bytes, verify stats); d_data == 0 is the size query (rc FCX_ERR_CAPACITY when there
        are RAW bytes).  check: raise on any rc but 0 and FCX_ERR_CAPACITY."""
        ne, nd = ctypes.c_uint32(), ctypes.c_uint64()
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        rc = lib().fcx_repair_build_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks,
                                          ctypes.c_void_p(d_orig or None), n, block_bytes, ctypes.c_void_p(d_entries or None),
                                          ctypes.c_void_p(d_data or None), data_cap, ctypes.byref(ne), ctypes.byref(nd), vals,
                                          ctypes.c_void_p(stream))
        if check and rc not in (0, -2):
            _check(rc, "fcx_repair_build_shard")
        return rc, int(ne.value), int(nd.value), self._verify_stats(vals)

    def repair_apply_shard(self, d_rec: int, rec_len: int, nblocks: int, kind: str, n: int, block_bytes: int, d_entries: int,
                           nentries: int, d_data: int, data_bytes: int, d_out: int, cap: int, stream: int = 0) -> int:
        """decodes the device records and applies the repair: the n original bytes to d_out; returns n"""
        out_len = ctypes.c_uint64()
        _check(lib().fcx_repair_apply_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, n,
                                            block_bytes, ctypes.c_void_p(d_entries or None), nentries,
                                            ctypes.c_void_p(d_data or None), data_bytes, ctypes.c_void_p(d_out or None), cap,
                                            ctypes.byref(out_len), ctypes.c_void_p(stream)), "fcx_repair_apply_shard")
        return int(out_len.value)

    def repair_stats(self) -> dict:
        """counters of the last repair call (fcx_dctx_repair_stats)"""
        n = len(self.REPAIR_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_repair_stats(self._h, vals, n), "fcx_dctx_repair_stats")
        return dict(zip(self.REPAIR_STATS, [int(v) for v in vals]))

    def repair_build_stream(self, src, orig, sink, block_bytes: int = BLOCK_BYTES, max_in: int = 0) -> dict:
        """a whole FCX7 or FCX8 file from src and the original from orig (binary readers) -> the canonical
        FCXR file to sink (a binary writer); returns the trailer: n, records, entries, data_bytes"""
        rd, _ = _stream_fns(src, None)
        ro, _ = _stream_fns(orig, None)
        _, wr = _stream_fns(None, sink)
        vals = (ctypes.c_uint64 * 4)()
        _check(lib().fcx_repair_build_stream(self._h, rd, None, ro, None, block_bytes, max_in, wr, None, vals),
               "fcx_repair_build_stream")
        return dict(zip(("n", "records", "entries", "data_bytes"), [int(v) for v in vals]))

    def repair_apply_stream(self, src, repair, sink, max_in: int = 0) -> int:
        """a whole FCX7 or FCX8 file from src and its FCXR file from repair -> the original bytes to sink"""
        rd, _ = _stream_fns(src, None)
        rr, _ = _stream_fns(repair, None)
        _, wr = _stream_fns(None, sink)
        total = ctypes.c_uint64()
        _check(lib().fcx_repair_apply_stream(self._h, rd, None, rr, None, wr, None, max_in, ctypes.byref(total)),
               "fcx_repair_apply_stream")
        return int(total.value)

    def repair_build_host(self, blob: bytes, data: bytes, block_bytes: int = BLOCK_BYTES) -> bytes:
        """the FCXR file of the whole file `blob` against `data`"""
        nrec = max(1, (len(data) + block_bytes - 1) // block_bytes)
        cap = REPAIR_HEADER_BYTES + REPAIR_TRAILER_BYTES + len(data) + (REPAIR_ENTRY_BYTES + 16) * nrec
        out = ctypes.create_string_buffer(cap)
        got = ctypes.c_uint64()
        _check(lib().fcx_repair_build_host(self._h, blob, len(blob), data, len(data), block_bytes, out, cap, ctypes.byref(got)),
               "fcx_repair_build_host")
        return out.raw[:got.value]

    def repair_apply_host(self, blob: bytes, repair: bytes, cap: int = None) -> bytes:
        """the whole file `blob` and its FCXR file -> the original bytes (cap defaults to the trailer's n)"""
        if cap is None:
            cap = struct.unpack_from("<Q", repair, len(repair) - REPAIR_TRAILER_BYTES + 8)[0] if len(repair) >= 56 else 0
            cap = min(cap, len(blob) // 7 * (BLOCK_BYTES + 8) + 8)   # (what the records can decode to at most)
        out = ctypes.create_string_buffer(max(cap, 1))
        got = ctypes.c_uint64()
        _check(lib().fcx_repair_apply_host(self._h, blob, len(blob), repair, len(repair), out, cap, ctypes.byref(got)),
               "fcx_repair_apply_host")
        return out.raw[:got.value]

    # ---- content digests (fcx_digest_* / fcx_check_*): a CRC-32 per block, and the test without the original ----
    DIGEST_STATS = ("segments", "bytes", "groups", "repaired")

    def digest_shard(self, d_data: int, n: int, block_bytes: int, d_crc: int, stream: int = 0, whole: bool = True):
        """the CRC-32 (zlib's) of every block of the n device bytes at d_data to d_crc (ceil(n / block_bytes)
        u32 on the device); returns the CRC-32 of all n bytes, or with whole=False None without waiting"""
        w = ctypes.c_uint32(0)
        _check(lib().fcx_digest_shard(self._h, ctypes.c_void_p(d_data or None), n, block_bytes, ctypes.c_void_p(d_crc or None),
                                      ctypes.byref(w) if whole else None, ctypes.c_void_p(stream)), "fcx_digest_shard")
        return int(w.value) if whole else None

    def digest_segments(self, d_data: int, d_off: int, nseg: int, d_crc: int, stream: int = 0):
        """the CRC-32 of the nseg segments [off[k], off[k + 1]) of d_data (d_off: nseg + 1 u64 on the device) to
        d_crc (nseg u32 on the device); enqueued on the stream"""
        _check(lib().fcx_digest_segments(self._h, ctypes.c_void_p(d_data or None), ctypes.c_void_p(d_off or None), nseg,
                                         ctypes.c_void_p(d_crc or None), ctypes.c_void_p(stream)), "fcx_digest_segments")

    def check_shard(self, d_rec: int, rec_len: int, nblocks: int, kind: str, n: int, block_bytes: int, d_crc: int,
                    d_entries: int = 0, nentries: int = 0, d_data: int = 0, data_bytes: int = 0, d_blocks: int = 0,
                    stream: int = 0) -> dict:
        """device records (no header), repaired by the given entries when there are any, against the CRC-32
        of the nblocks blocks of the n bytes they were compressed from (d_crc, u32 on the device); d_blocks
        (2 * nblocks u32 on the device, or 0) receives per record the resulting length and CRC-32.  Returns
        the stats: blocks, differ (the failing blocks), first, size_differs, bytes, decoded."""
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        _check(lib().fcx_check_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, n, block_bytes,
                                     ctypes.c_void_p(d_entries or None), nentries, ctypes.c_void_p(d_data or None), data_bytes,
                                     ctypes.c_void_p(d_crc or None), ctypes.c_void_p(d_blocks or None), vals,
                                     ctypes.c_void_p(stream)), "fcx_check_shard")
        return self._verify_stats(vals)

    def digest_stats(self) -> dict:
        """counters of the last digest or check call (fcx_dctx_digest_stats)"""
        n = len(self.DIGEST_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_digest_stats(self._h, vals, n), "fcx_dctx_digest_stats")
        return dict(zip(self.DIGEST_STATS, [int(v) for v in vals]))

    def set_digest_slice(self, nbytes: int):
        """testing and timing: bytes per slicing round of the CRC kernel in later calls (4, 8, 16; 0: the default)"""
        _check(lib().fcx_dctx_set_digest_slice(self._h, nbytes), "fcx_dctx_set_digest_slice")

    def digest_stream(self, orig, sink, block_bytes: int = BLOCK_BYTES) -> dict:
        """the original from orig (a binary reader) -> its canonical FCXD file to sink (a binary writer);
        returns the trailer: n, blocks, crc32"""
        ro, _ = _stream_fns(orig, None)
        _, wr = _stream_fns(None, sink)
        vals = (ctypes.c_uint64 * 3)()
        _check(lib().fcx_digest_stream(self._h, ro, None, block_bytes, wr, None, vals), "fcx_digest_stream")
        return dict(zip(("n", "blocks", "crc32"), [int(v) for v in vals]))

    def check_stream(self, src, digest, repair=None, max_in: int = 0):
        """a whole FCX7 or FCX8 file from src, its FCXD file from digest and, when given, its FCXR file from
        repair (binary readers); returns (stats, [(block, its length by the digest file, resulting length,
        resulting CRC-32)] of the failing blocks).  Blocks of the digest file behind the last record come
        last, as block number stats["blocks"] with their bytes.  The file passes when stats["differ"] == 0 and
        stats["bytes"] == 0."""
        rd, _ = _stream_fns(src, None)
        rg, _ = _stream_fns(digest, None)
        rr = _stream_fns(repair, None)[0] if repair is not None else ctypes.cast(None, READ_FN)
        bad = []
        cb = VERIFY_FN(lambda _u, k, blen, got, crc: bad.append((int(k), int(blen), int(got), int(crc))))
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        _check(lib().fcx_check_stream(self._h, rd, None, rr, None, rg, None, max_in, cb, None, vals), "fcx_check_stream")
        return self._verify_stats(vals), bad

    def digest_host(self, data: bytes, block_bytes: int = BLOCK_BYTES) -> bytes:
        """the FCXD file of `data` in blocks of block_bytes"""
        nb = (len(data) + block_bytes - 1) // block_bytes
        cap = DIGEST_HEADER_BYTES + DIGEST_TRAILER_BYTES + 8 + 4 * nb + 8 * (nb // DIGEST_SECTION + 1)
        out = ctypes.create_string_buffer(cap)
        got = ctypes.c_uint64()
        _check(lib().fcx_digest_host(self._h, data, len(data), block_bytes, out, cap, ctypes.byref(got)), "fcx_digest_host")
        return out.raw[:got.value]

    def check_host(self, blob: bytes, digest: bytes, repair: bytes = None):
        """check_stream on memory: the whole file `blob`, its FCXD file and, when given, its FCXR file"""
        bad = []
        cb = VERIFY_FN(lambda _u, k, blen, got, crc: bad.append((int(k), int(blen), int(got), int(crc))))
        vals = (ctypes.c_uint64 * len(self.VERIFY_STATS))()
        _check(lib().fcx_check_host(self._h, blob, len(blob), repair, len(repair) if repair is not None else 0, digest,
                                    len(digest), cb, None, vals), "fcx_check_host")
        return self._verify_stats(vals), bad

    # ---- search (fcx_find_*): where a byte string occurs in the decoded run ----
    FIND_STATS = ("judged", "candidates", "hits", "groups", "carry_bytes", "windows")

    def find_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, pattern: bytes, d_hits: int = 0, cap: int = 0,
                   stream: int = 0) -> int:
        """searches device records (no header) for `pattern` (1 to 256 bytes); returns the number of hits in
        the run; the first min(cap, hits) offsets go to d_hits (u64 on the device), ascending"""
        n = ctypes.c_uint64(0)
        _check(lib().fcx_find_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, pattern, len(pattern),
                                    ctypes.c_void_p(d_hits or None), cap, ctypes.byref(n), ctypes.c_void_p(stream)),
               "fcx_find_shard")
        return int(n.value)

    def find(self, blob: bytes, pattern: bytes, max_hits: int = None):
        """a whole FCX7 or FCX8 file in memory -> (count, [offsets]): every offset of the decoded file at which
        `pattern` occurs, ascending, the first max_hits of them when that is given (0: the count alone)"""
        n = ctypes.c_uint64(0)
        if not max_hits:   # the count: all there is to do, or what sizes the room for all
            _check(lib().fcx_find_host(self._h, blob, len(blob), pattern, len(pattern), None, 0, ctypes.byref(n)), "fcx_find_host")
            if max_hits == 0 or n.value == 0:
                return int(n.value), []
            max_hits = int(n.value)
        out = (ctypes.c_uint64 * max_hits)()
        _check(lib().fcx_find_host(self._h, blob, len(blob), pattern, len(pattern), out, max_hits, ctypes.byref(n)), "fcx_find_host")
        return int(n.value), [int(v) for v in out[:min(max_hits, int(n.value))]]

    def find_stats(self) -> dict:
        """counters of the last find call (fcx_dctx_find_stats)"""
        n = len(self.FIND_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_find_stats(self._h, vals, n), "fcx_dctx_find_stats")
        return dict(zip(self.FIND_STATS, [int(v) for v in vals]))

    def set_find_window(self, hits: int):
        """testing: hits per window of the stream form's hit buffer in later calls (0: the default)"""
        _check(lib().fcx_dctx_set_find_window(self._h, hits), "fcx_dctx_set_find_window")

    # ---- grep (fcx_grep_*, fcx_decompress_ranges_*): the lines that hold a byte string, and many ranges in one call ----
    GREP_STATS = ("lines", "bytes", "hits", "judged", "decoded")
    RANGES_STATS = ("ranges", "bytes", "records_touched", "records_decoded", "groups")

    def grep_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, pattern: bytes, delim=b"\n", d_start: int = 0,
                   d_end: int = 0, cap: int = 0, stream: int = 0) -> dict:
        """the lines of device records (no header) that hold `pattern` (1 to 256 bytes without the delimiter): returns
        {lines, bytes, hits, judged, decoded}; start and end of the first min(cap, lines) go to d_start / d_end (u64
        on the device, two arrays), ascending"""
        vals = (ctypes.c_uint64 * len(self.GREP_STATS))()
        _check(lib().fcx_grep_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, self._delim(delim),
                                    pattern, len(pattern), ctypes.c_void_p(d_start or None), ctypes.c_void_p(d_end or None), cap, vals,
                                    ctypes.c_void_p(stream)), "fcx_grep_shard")
        return dict(zip(self.GREP_STATS, [int(v) for v in vals]))

    def decompress_ranges_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, d_start: int, d_end: int, nranges: int,
                                d_out: int, cap: int, index=None, stream: int = 0) -> int:
        """the decoded bytes of nranges ascending, disjoint ranges [d_start[i], d_end[i]) (u64 on the device) back to
        back to d_out[0 ..); returns their count; index: the device arrays (rec_off, dec_off) of index_shard, or None"""
        got = ctypes.c_uint64(0)
        ro, do = index if index is not None else (0, 0)
        _check(lib().fcx_decompress_ranges_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks,
                                                 ctypes.c_void_p(ro or None), ctypes.c_void_p(do or None), ctypes.c_void_p(d_start or None),
                                                 ctypes.c_void_p(d_end or None), nranges, ctypes.c_void_p(d_out or None), cap,
                                                 ctypes.byref(got), ctypes.c_void_p(stream)), "fcx_decompress_ranges_shard")
        return int(got.value)

    def ranges_stats(self) -> dict:
        """counters of the last decompress_ranges_shard call (fcx_dctx_ranges_stats)"""
        n = len(self.RANGES_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_ranges_stats(self._h, vals, n), "fcx_dctx_ranges_stats")
        return dict(zip(self.RANGES_STATS, [int(v) for v in vals]))

    def grep_scratch(self) -> int:
        """device bytes the last grep_shard call reserved beside the decoded group: bitmaps and tile words"""
        v = ctypes.c_uint64(0)
        _check(lib().fcx_dctx_grep_scratch(self._h, ctypes.byref(v)), "fcx_dctx_grep_scratch")
        return int(v.value)

    def grep_host(self, blob: bytes, pattern: bytes, delim=b"\n"):
        """a whole FCX7 or FCX8 file in memory -> (stats, the bytes of the lines that hold `pattern`): grep -F; the
        lines are found and gathered on the GPU, only their bytes come back"""
        vals = (ctypes.c_uint64 * len(self.GREP_STATS))()
        need = ctypes.c_uint64(0)
        args = (self._h, blob, len(blob), self._delim(delim), pattern, len(pattern))
        rc = lib().fcx_grep_host(*args, None, 0, ctypes.byref(need), vals)   # the size
        if rc != -2:
            _check(rc, "fcx_grep_host")
            return dict(zip(self.GREP_STATS, [int(v) for v in vals])), b""
        out = ctypes.create_string_buffer(need.value)
        _check(lib().fcx_grep_host(*args, out, need.value, ctypes.byref(need), vals), "fcx_grep_host")
        return dict(zip(self.GREP_STATS, [int(v) for v in vals])), out.raw[:need.value]

    def decompress_ranges_host(self, blob: bytes, ranges) -> bytes:
        """the decoded bytes of the ascending, disjoint (start, end) pairs of a whole FCX7 or FCX8 file, back to back"""
        n = len(ranges)
        starts = (ctypes.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        ends = (ctypes.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        cap = sum(max(e - s, 0) for s, e in ranges)
        out = ctypes.create_string_buffer(max(cap, 1))
        got = ctypes.c_uint64(0)
        _check(lib().fcx_decompress_ranges_host(self._h, blob, len(blob), starts, ends, n, out, cap, ctypes.byref(got)),
               "fcx_decompress_ranges_host")
        return out.raw[:got.value]

    def grep_stream(self, src, pattern: bytes, delim=b"\n", max_in: int = 0, want_lines: bool = True):
        """an FCX7 or FCX8 file from src (binary reader) -> (stats, [(start, end)] of every line that holds `pattern`,
        ascending, each once and with its true end); want_lines False: the totals alone"""
        rd, _ = _stream_fns(src, None)
        got = []
        cb = RANGE_FN(lambda _u, s, e: got.append((int(s), int(e)))) if want_lines else ctypes.cast(None, RANGE_FN)
        vals = (ctypes.c_uint64 * len(self.GREP_STATS))()
        _check(lib().fcx_grep_stream(self._h, rd, None, max_in, self._delim(delim), pattern, len(pattern), cb, None, vals),
               "fcx_grep_stream")
        return dict(zip(self.GREP_STATS, [int(v) for v in vals])), got

    def decompress_ranges_stream(self, src, sink, ranges, max_in: int = 0) -> int:
        """the decoded bytes of the ascending, disjoint (start, end) pairs of an FCX7 or FCX8 file from src (binary
        reader) to sink, back to back; reads no further than the last range needs; returns the bytes written"""
        rd, wr = _stream_fns(src, sink)
        n = len(ranges)
        starts = (ctypes.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        ends = (ctypes.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        got = ctypes.c_uint64(0)
        _check(lib().fcx_decompress_ranges_stream(self._h, rd, wr, None, max_in, starts, ends, n, ctypes.byref(got)),
               "fcx_decompress_ranges_stream")
        return int(got.value)

    # ---- pattern sets (fcx_*_set_*): up to 64 patterns, with or without ASCII case folding, in one scan ----
    SET_SCAN_STATS = ("judged", "candidates", "compares", "hits", "groups", "final_passes")

    def find_set_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, pset: "PatternSet", d_hits: int = 0, cap: int = 0,
                       stream: int = 0):
        """searches device records (no header) for the patterns of `pset`; returns (hits, counts): the positions at
        which at least one occurs and, per pattern, the positions at which it does; the first min(cap, hits) offsets
        go to d_hits (u64 on the device), ascending, each once"""
        n = ctypes.c_uint64(0)
        counts = (ctypes.c_uint64 * len(pset))()
        _check(lib().fcx_find_set_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, pset.handle,
                                        ctypes.c_void_p(d_hits or None), cap, ctypes.byref(n), counts, ctypes.c_void_p(stream)),
               "fcx_find_set_shard")
        return int(n.value), [int(v) for v in counts]

    def find_set(self, blob: bytes, pset: "PatternSet", max_hits: int = None):
        """a whole FCX7 or FCX8 file in memory -> (count, [offsets], counts): every offset of the decoded file at which
        a pattern of `pset` occurs, ascending, the first max_hits of them when that is given (0: the counts alone)"""
        n = ctypes.c_uint64(0)
        counts = (ctypes.c_uint64 * len(pset))()
        if not max_hits:
            _check(lib().fcx_find_set_host(self._h, blob, len(blob), pset.handle, None, 0, ctypes.byref(n), counts), "fcx_find_set_host")
            if max_hits == 0 or n.value == 0:
                return int(n.value), [], [int(v) for v in counts]
            max_hits = int(n.value)
        out = (ctypes.c_uint64 * max_hits)()
        _check(lib().fcx_find_set_host(self._h, blob, len(blob), pset.handle, out, max_hits, ctypes.byref(n), counts), "fcx_find_set_host")
        return int(n.value), [int(v) for v in out[:min(max_hits, int(n.value))]], [int(v) for v in counts]

    def find_set_stream(self, src, pset: "PatternSet", max_in: int = 0, want_hits: bool = True):
        """an FCX7 or FCX8 file from src (binary reader) -> ({hits, decoded, records, judged}, [offsets], counts)"""
        rd, _ = _stream_fns(src, None)
        got = []
        cb = HIT_FN(lambda _u, off: got.append(int(off))) if want_hits else ctypes.cast(None, HIT_FN)
        vals = (ctypes.c_uint64 * 4)()
        counts = (ctypes.c_uint64 * len(pset))()
        _check(lib().fcx_find_set_stream(self._h, rd, None, max_in, pset.handle, cb, None, vals, counts), "fcx_find_set_stream")
        return dict(zip(("hits", "decoded", "records", "judged"), [int(v) for v in vals])), got, [int(v) for v in counts]

    def grep_set_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, pset: "PatternSet", delim=b"\n", d_start: int = 0,
                       d_end: int = 0, cap: int = 0, stream: int = 0):
        """the lines of device records (no header) that hold a pattern of `pset`: returns ({lines, bytes, hits, judged,
        decoded}, counts); start and end of the first min(cap, lines) go to d_start / d_end (u64 on the device)"""
        vals = (ctypes.c_uint64 * len(self.GREP_STATS))()
        counts = (ctypes.c_uint64 * len(pset))()
        _check(lib().fcx_grep_set_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, self._delim(delim),
                                        pset.handle, ctypes.c_void_p(d_start or None), ctypes.c_void_p(d_end or None), cap, vals, counts,
                                        ctypes.c_void_p(stream)), "fcx_grep_set_shard")
        return dict(zip(self.GREP_STATS, [int(v) for v in vals])), [int(v) for v in counts]

    def grep_set_host(self, blob: bytes, pset: "PatternSet", delim=b"\n"):
        """a whole FCX7 or FCX8 file in memory -> (stats, the bytes of the lines that hold a pattern of `pset`, counts):
        grep -F -f; the lines are found and gathered on the GPU, only their bytes come back"""
        vals = (ctypes.c_uint64 * len(self.GREP_STATS))()
        counts = (ctypes.c_uint64 * len(pset))()
        need = ctypes.c_uint64(0)
        args = (self._h, blob, len(blob), self._delim(delim), pset.handle)
        rc = lib().fcx_grep_set_host(*args, None, 0, ctypes.byref(need), vals, counts)   # the size
        if rc != -2:
            _check(rc, "fcx_grep_set_host")
            return dict(zip(self.GREP_STATS, [int(v) for v in vals])), b"", [int(v) for v in counts]
        out = ctypes.create_string_buffer(need.value)
        _check(lib().fcx_grep_set_host(*args, out, need.value, ctypes.byref(need), vals, counts), "fcx_grep_set_host")
        return dict(zip(self.GREP_STATS, [int(v) for v in vals])), out.raw[:need.value], [int(v) for v in counts]

    def grep_set_stream(self, src, pset: "PatternSet", delim=b"\n", max_in: int = 0, want_lines: bool = True):
        """an FCX7 or FCX8 file from src (binary reader) -> (stats, [(start, end)] of every line that holds a pattern of
        `pset`, ascending, each once and with its true end, counts); want_lines False: the totals alone"""
        rd, _ = _stream_fns(src, None)
        got = []
        cb = RANGE_FN(lambda _u, s, e: got.append((int(s), int(e)))) if want_lines else ctypes.cast(None, RANGE_FN)
        vals = (ctypes.c_uint64 * len(self.GREP_STATS))()
        counts = (ctypes.c_uint64 * len(pset))()
        _check(lib().fcx_grep_set_stream(self._h, rd, None, max_in, self._delim(delim), pset.handle, cb, None, vals, counts),
               "fcx_grep_set_stream")
        return dict(zip(self.GREP_STATS, [int(v) for v in vals])), got, [int(v) for v in counts]

    # ---- context and inverted grep (fcx_grep_blocks_*): grep -v / -A / -B / -C as blocks of consecutive selected lines ----
    GREP_BLOCK_STATS = ("blocks", "lines", "bytes", "base_lines", "hits", "judged", "decoded", "total_lines")
    GREP_INVERT = 1
    GREP_MAX_CONTEXT = 4096

    @classmethod
    def _opts(cls, invert, before, after) -> "GrepOpts":
        if not (0 <= before < 1 << 32 and 0 <= after < 1 << 32):
            raise ValueError("before and after are counts of lines")
        return GrepOpts(cls.GREP_INVERT if invert else 0, before, after)

    def grep_blocks_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, pset: "PatternSet", delim=b"\n", invert: bool = False,
                          before: int = 0, after: int = 0, d_start: int = 0, d_end: int = 0, d_line: int = 0, cap: int = 0,
                          stream: int = 0):
        """the blocks of device records (no header): the maximal runs of lines that hold a pattern of `pset` (invert: that
        hold none) or lie within `before` lines in front of or `after` lines behind such a line.  Returns
        (GREP_BLOCK_STATS, counts); start, end and first line of the first min(cap, blocks) go to d_start / d_end /
        d_line (u64 on the device)"""
        vals = (ctypes.c_uint64 * len(self.GREP_BLOCK_STATS))()
        counts = (ctypes.c_uint64 * len(pset))()
        opts = self._opts(invert, before, after)
        _check(lib().fcx_grep_blocks_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, self._delim(delim),
                                           pset.handle, ctypes.byref(opts), ctypes.c_void_p(d_start or None),
                                           ctypes.c_void_p(d_end or None), ctypes.c_void_p(d_line or None), cap, vals, counts,
                                           ctypes.c_void_p(stream)), "fcx_grep_blocks_shard")
        return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), [int(v) for v in counts]

    def grep_blocks_host(self, blob: bytes, pset: "PatternSet", delim=b"\n", invert: bool = False, before: int = 0, after: int = 0):
        """a whole FCX7 or FCX8 file in memory -> (stats, the blocks' bytes concatenated, counts): grep -F -f with -v, -B
        and -A, without the `--` lines; found and gathered on the GPU, only the blocks' bytes come back"""
        vals = (ctypes.c_uint64 * len(self.GREP_BLOCK_STATS))()
        counts = (ctypes.c_uint64 * len(pset))()
        need = ctypes.c_uint64(0)
        opts = self._opts(invert, before, after)
        args = (self._h, blob, len(blob), self._delim(delim), pset.handle, ctypes.byref(opts))
        rc = lib().fcx_grep_blocks_host(*args, None, 0, ctypes.byref(need), vals, counts)   # the size
        if rc != -2:
            _check(rc, "fcx_grep_blocks_host")
            return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), b"", [int(v) for v in counts]
        out = ctypes.create_string_buffer(need.value)
        _check(lib().fcx_grep_blocks_host(*args, out, need.value, ctypes.byref(need), vals, counts), "fcx_grep_blocks_host")
        return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), out.raw[:need.value], [int(v) for v in counts]

    def grep_blocks_stream(self, src, pset: "PatternSet", delim=b"\n", invert: bool = False, before: int = 0, after: int = 0,
                           max_in: int = 0, want_blocks: bool = True):
        """an FCX7 or FCX8 file from src (binary reader) -> (stats, [(start, end, line, nlines)] of every block, ascending,
        each once and with its true end, counts); want_blocks False: the totals alone"""
        rd, _ = _stream_fns(src, None)
        got = []
        cb = BLOCK_FN(lambda _u, s, e, ln, n: got.append((int(s), int(e), int(ln), int(n)))) if want_blocks else ctypes.cast(None, BLOCK_FN)
        vals = (ctypes.c_uint64 * len(self.GREP_BLOCK_STATS))()
        counts = (ctypes.c_uint64 * len(pset))()
        opts = self._opts(invert, before, after)
        _check(lib().fcx_grep_blocks_stream(self._h, rd, None, max_in, self._delim(delim), pset.handle, ctypes.byref(opts), cb, None, vals,
                                            counts), "fcx_grep_blocks_stream")
        return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), got, [int(v) for v in counts]

    # ---- regular-expression grep (fcx_grep_regex_blocks_*): grep -E with -v / -A / -B / -C; the delimiter is the regex's ----
    REGEX_SCAN_STATS = ("judged", "hits", "groups", "final_passes")

    def grep_regex_blocks_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, regex: "Regex", invert: bool = False,
                                before: int = 0, after: int = 0, d_start: int = 0, d_end: int = 0, d_line: int = 0, cap: int = 0,
                                stream: int = 0) -> dict:
        """grep_blocks_shard with a Regex for the set: the blocks of the lines in which a match of `regex` ends.  Returns
        GREP_BLOCK_STATS; start, end and first line of the first min(cap, blocks) go to d_start / d_end / d_line"""
        vals = (ctypes.c_uint64 * len(self.GREP_BLOCK_STATS))()
        opts = self._opts(invert, before, after)
        _check(lib().fcx_grep_regex_blocks_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, regex.handle,
                                                 ctypes.byref(opts), ctypes.c_void_p(d_start or None), ctypes.c_void_p(d_end or None),
                                                 ctypes.c_void_p(d_line or None), cap, vals, ctypes.c_void_p(stream)),
               "fcx_grep_regex_blocks_shard")
        return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals]))

    def grep_regex_blocks_host(self, blob: bytes, regex: "Regex", invert: bool = False, before: int = 0, after: int = 0):
        """a whole FCX7 or FCX8 file in memory -> (stats, the blocks' bytes concatenated): grep -E with -v, -B and -A,
        without the `--` lines; found and gathered on the GPU, only the blocks' bytes come back"""
        vals = (ctypes.c_uint64 * len(self.GREP_BLOCK_STATS))()
        need = ctypes.c_uint64(0)
        opts = self._opts(invert, before, after)
        args = (self._h, blob, len(blob), regex.handle, ctypes.byref(opts))
        rc = lib().fcx_grep_regex_blocks_host(*args, None, 0, ctypes.byref(need), vals)   # the size
        if rc != -2:
            _check(rc, "fcx_grep_regex_blocks_host")
            return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), b""
        out = ctypes.create_string_buffer(need.value)
        _check(lib().fcx_grep_regex_blocks_host(*args, out, need.value, ctypes.byref(need), vals), "fcx_grep_regex_blocks_host")
        return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), out.raw[:need.value]

    def grep_regex_blocks_stream(self, src, regex: "Regex", invert: bool = False, before: int = 0, after: int = 0, max_in: int = 0,
                                 want_blocks: bool = True):
        """an FCX7 or FCX8 file from src (binary reader) -> (stats, [(start, end, line, nlines)] of every block, ascending,
        each once and with its true end); want_blocks False: the totals alone"""
        rd, _ = _stream_fns(src, None)
        got = []
        cb = BLOCK_FN(lambda _u, s, e, ln, n: got.append((int(s), int(e), int(ln), int(n)))) if want_blocks else ctypes.cast(None, BLOCK_FN)
        vals = (ctypes.c_uint64 * len(self.GREP_BLOCK_STATS))()
        opts = self._opts(invert, before, after)
        _check(lib().fcx_grep_regex_blocks_stream(self._h, rd, None, max_in, regex.handle, ctypes.byref(opts), cb, None, vals),
               "fcx_grep_regex_blocks_stream")
        return dict(zip(self.GREP_BLOCK_STATS, [int(v) for v in vals])), got

    def regex_scan_stats(self) -> dict:
        """counters of the last regex call (fcx_dctx_regex_scan_stats)"""
        n = len(self.REGEX_SCAN_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_regex_scan_stats(self._h, vals, n), "fcx_dctx_regex_scan_stats")
        return dict(zip(self.REGEX_SCAN_STATS, [int(v) for v in vals]))

    # ---- cut (fcx_cut_*): fields and byte columns of the lines of the decoded run; the rule and its two differences
    # from GNU cut: include/fcx.h.  Every device call returns (total, stats): d_out receives the first min(cap, total)
    # bytes, d_out 0 with cap 0 is the size query ----
    CUT_STATS = ("out_bytes", "judged", "delimiters", "separators", "separators_kept", "groups")

    def _cut_out(self, rc, what, total, vals):
        _check(rc, what)
        return int(total.value), dict(zip(self.CUT_STATS, [int(v) for v in vals]))

    def cut_buffer(self, d_in: int, n: int, cut: "Cut", d_out: int = 0, cap: int = 0, stream: int = 0):
        """cuts the n plain device bytes at d_in as one text; any alignment of d_in and d_out"""
        vals, total = (ctypes.c_uint64 * len(self.CUT_STATS))(), ctypes.c_uint64(0)
        rc = lib().fcx_cut_buffer(self._h, ctypes.c_void_p(d_in or None), n, cut.handle, ctypes.c_void_p(d_out or None), cap,
                                  ctypes.byref(total), vals, ctypes.c_void_p(stream))
        return self._cut_out(rc, "fcx_cut_buffer", total, vals)

    def cut_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, cut: "Cut", d_out: int = 0, cap: int = 0, stream: int = 0):
        """cuts what the nblocks records at d_rec decode to, group by group on the device"""
        vals, total = (ctypes.c_uint64 * len(self.CUT_STATS))(), ctypes.c_uint64(0)
        rc = lib().fcx_cut_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, cut.handle,
                                 ctypes.c_void_p(d_out or None), cap, ctypes.byref(total), vals, ctypes.c_void_p(stream))
        return self._cut_out(rc, "fcx_cut_shard", total, vals)

    def cut_ranges_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, d_start: int, d_end: int, nranges: int, cut: "Cut",
                         d_out: int = 0, cap: int = 0, index=None, stream: int = 0):
        """cuts the concatenation of the ranges [d_start[i], d_end[i]) (u64 on the device; a grep's lines or blocks) as
        one text; index: the device arrays (rec_off, dec_off) of index_shard, or None"""
        vals, total = (ctypes.c_uint64 * len(self.CUT_STATS))(), ctypes.c_uint64(0)
        ro, do = index if index is not None else (0, 0)
        rc = lib().fcx_cut_ranges_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, ctypes.c_void_p(ro or None),
                                        ctypes.c_void_p(do or None), ctypes.c_void_p(d_start or None), ctypes.c_void_p(d_end or None),
                                        nranges, cut.handle, ctypes.c_void_p(d_out or None), cap, ctypes.byref(total), vals,
                                        ctypes.c_void_p(stream))
        return self._cut_out(rc, "fcx_cut_ranges_shard", total, vals)

    def cut_stream(self, src, sink, cut: "Cut", max_in: int = 0) -> dict:
        """an FCX7 or FCX8 file from src (binary reader), its cut to sink (binary writer; None: the totals alone)"""
        rd, wr = _stream_fns(src, sink)
        vals = (ctypes.c_uint64 * len(self.CUT_STATS))()
        _check(lib().fcx_cut_stream(self._h, rd, wr if sink is not None else ctypes.cast(None, WRITE_FN), None, max_in, cut.handle, vals),
               "fcx_cut_stream")
        return dict(zip(self.CUT_STATS, [int(v) for v in vals]))

    def _cut_host(self, fn, what, args, size_only, room=None):
        """room: bytes that hold the output whatever it is (one call); None: the size query first, then the call"""
        vals, need = (ctypes.c_uint64 * len(self.CUT_STATS))(), ctypes.c_uint64(0)
        if room is None or size_only:
            rc = fn(*args, None, 0, ctypes.byref(need), vals)   # the size
            if rc != -2 or size_only:
                if rc != -2:
                    _check(rc, what)
                return int(need.value), dict(zip(self.CUT_STATS, [int(v) for v in vals])), b""
            room = need.value
        out = ctypes.create_string_buffer(max(room, 1))
        _check(fn(*args, out, room, ctypes.byref(need), vals), what)
        return int(need.value), dict(zip(self.CUT_STATS, [int(v) for v in vals])), out.raw[:need.value]

    def cut_host(self, blob: bytes, cut: "Cut", size_only: bool = False):
        """a whole FCX7 or FCX8 file in memory -> (total, stats, the cut's bytes; b"" with size_only).  Without size_only
        the file is decoded and cut twice: the size query (no gather), then the call into a buffer of that size"""
        return self._cut_host(lib().fcx_cut_host, "fcx_cut_host", (self._h, blob, len(blob), cut.handle), size_only)

    def cut_ranges_host(self, blob: bytes, ranges, cut: "Cut", size_only: bool = False):
        """cut_host over the ascending, disjoint (start, end) pairs of what the file decodes to"""
        n = len(ranges)
        starts = (ctypes.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        ends = (ctypes.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        room = sum(max(e - s, 0) for s, e in ranges)   # (the cut is a subsequence of the ranges' bytes: one call)
        return self._cut_host(lib().fcx_cut_ranges_host, "fcx_cut_ranges_host", (self._h, blob, len(blob), starts, ends, n, cut.handle),
                              size_only, room)

    def cut_stats(self) -> dict:
        """counters of the last cut call (fcx_dctx_cut_stats)"""
        n = len(self.CUT_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_cut_stats(self._h, vals, n), "fcx_dctx_cut_stats")
        return dict(zip(self.CUT_STATS, [int(v) for v in vals]))

    def cut_scratch(self) -> int:
        """device bytes the last cut call reserved beside the decoded group"""
        v = ctypes.c_uint64(0)
        _check(lib().fcx_dctx_cut_scratch(self._h, ctypes.byref(v)), "fcx_dctx_cut_scratch")
        return int(v.value)

    def set_scan_stats(self) -> dict:
        """counters of the last pattern-set call (fcx_dctx_set_scan_stats)"""
        n = len(self.SET_SCAN_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_set_scan_stats(self._h, vals, n), "fcx_dctx_set_scan_stats")
        return dict(zip(self.SET_SCAN_STATS, [int(v) for v in vals]))

    # ---- lines (fcx_lines_*): count, locate, decode and number the lines of the decoded run; lines are 0-based,
    # delim is one byte, count None means "to the end" ----
    LINES_STATS = ("delimiters", "lines", "decoded", "tail_bytes")
    LINES_CALL_STATS = ("bytes_counted", "records", "groups", "offsets_ranked", "selects")

    @staticmethod
    def _delim(delim) -> int:
        if isinstance(delim, int):
            if not 0 <= delim <= 255:
                raise ValueError("the delimiter is one byte")
            return delim
        if len(delim) != 1:
            raise ValueError("the delimiter is one byte")
        return delim[0]

    def lines_index_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, delim=b"\n", d_line_off: int = 0,
                          stream: int = 0) -> dict:
        """the line column of the index: d_line_off[k] = delimiters in front of record k (nblocks + 1 u64 on the
        device, or 0 for the counts alone); returns {delimiters, lines, decoded, tail_bytes}"""
        vals = (ctypes.c_uint64 * len(self.LINES_STATS))()
        _check(lib().fcx_lines_index_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks,
                                           self._delim(delim), ctypes.c_void_p(d_line_off or None), vals, ctypes.c_void_p(stream)),
               "fcx_lines_index_shard")
        return dict(zip(self.LINES_STATS, [int(v) for v in vals]))

    def lines_locate_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, first: int, count: int = None, delim=b"\n",
                           index=None, stream: int = 0):
        """(offset, length) of lines [first, first + count) in the decoded run; index: the three device arrays
        (rec_off, dec_off, line_off) of index_shard and lines_index_shard, or None (the call counts itself)"""
        off, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
        ro, do, lo = index if index is not None else (0, 0, 0)
        _check(lib().fcx_lines_locate_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks,
                                            self._delim(delim), ctypes.c_void_p(ro or None), ctypes.c_void_p(do or None),
                                            ctypes.c_void_p(lo or None), first, 2**64 - 1 if count is None else count,
                                            ctypes.byref(off), ctypes.byref(n), ctypes.c_void_p(stream)), "fcx_lines_locate_shard")
        return int(off.value), int(n.value)

    def decompress_lines_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, first: int, count: int, d_out: int,
                               cap: int, delim=b"\n", index=None, stream: int = 0) -> int:
        """the bytes of lines [first, first + count) to d_out[0 ..); returns their count"""
        got = ctypes.c_uint64(0)
        ro, do, lo = index if index is not None else (0, 0, 0)
        _check(lib().fcx_decompress_lines_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks,
                                                self._delim(delim), ctypes.c_void_p(ro or None), ctypes.c_void_p(do or None),
                                                ctypes.c_void_p(lo or None), first, 2**64 - 1 if count is None else count,
                                                ctypes.c_void_p(d_out or None), cap, ctypes.byref(got), ctypes.c_void_p(stream)),
               "fcx_decompress_lines_shard")
        return int(got.value)

    def lines_of_shard(self, kind: str, d_rec: int, rec_len: int, nblocks: int, d_offsets: int, noff: int, d_lines: int,
                       delim=b"\n", stream: int = 0):
        """d_lines[i] = the line of d_offsets[i] for noff ascending decoded offsets on the device (find_shard's d_hits)"""
        _check(lib().fcx_lines_of_shard(self._h, kind.encode(), ctypes.c_void_p(d_rec or None), rec_len, nblocks, self._delim(delim),
                                        ctypes.c_void_p(d_offsets or None), noff, ctypes.c_void_p(d_lines or None),
                                        ctypes.c_void_p(stream)), "fcx_lines_of_shard")

    def count_lines(self, blob: bytes, delim=b"\n") -> dict:
        """a whole FCX7 or FCX8 file in memory -> {delimiters, lines, decoded, tail_bytes} (wc -l)"""
        vals = (ctypes.c_uint64 * len(self.LINES_STATS))()
        _check(lib().fcx_lines_host(self._h, blob, len(blob), self._delim(delim), vals), "fcx_lines_host")
        return dict(zip(self.LINES_STATS, [int(v) for v in vals]))

    def lines_locate(self, blob: bytes, first: int, count: int = None, delim=b"\n"):
        """(offset, length) of lines [first, first + count) in what a whole FCX7 or FCX8 file decodes to: one pass
        (fcx_lines_locate_stream), which ends once both boundaries are known"""
        import io

        rd, _ = _stream_fns(io.BytesIO(blob), None)
        off, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().fcx_lines_locate_stream(self._h, rd, None, max(0, len(blob) - HEADER_BYTES), self._delim(delim), first,
                                             2**64 - 1 if count is None else count, ctypes.byref(off), ctypes.byref(n)),
               "fcx_lines_locate_stream")
        return int(off.value), int(n.value)

    def decompress_lines(self, blob: bytes, first: int, count: int = None, delim=b"\n") -> bytes:
        """the bytes of lines [first, first + count) of a whole FCX7 or FCX8 file (sed -n): the locate once, then the
        range decode of what it found"""
        off, n = self.lines_locate(blob, first, count, delim)
        return self.decompress_range_host(blob, off, n) if n else b""

    def line_numbers(self, blob: bytes, offsets, delim=b"\n"):
        """the line (0-based) of each of the ascending decoded offsets of a whole FCX7 or FCX8 file"""
        n = len(offsets)
        offs = (ctypes.c_uint64 * max(n, 1))(*offsets)
        out = (ctypes.c_uint64 * max(n, 1))()
        _check(lib().fcx_lines_of_host(self._h, blob, len(blob), self._delim(delim), offs, n, out), "fcx_lines_of_host")
        return [int(v) for v in out[:n]]

    def lines_stats(self) -> dict:
        """counters of the last line call (fcx_dctx_lines_stats)"""
        n = len(self.LINES_CALL_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_lines_stats(self._h, vals, n), "fcx_dctx_lines_stats")
        return dict(zip(self.LINES_CALL_STATS, [int(v) for v in vals]))

    def set_profiling(self, on: bool = True):
        _check(lib().fcx_dctx_set_profiling(self._h, 1 if on else 0), "fcx_dctx_set_profiling")

    def stage_times(self):
        res = []
        for i in range(lib().fcx_dctx_stage_count(self._h)):
            name = ctypes.c_char_p()
            ms = ctypes.c_float()
            _check(lib().fcx_dctx_stage(self._h, i, ctypes.byref(name), ctypes.byref(ms)), "fcx_dctx_stage")
            res.append((name.value.decode(), ms.value))
        return res

    SYMBOL_STATS = ("rounds", "fallbacks", "fallbacks_flags", "fallbacks_chars", "fallbacks_p",
                    "fallbacks_golomb_bytes", "golomb_rounds", "golomb_fallbacks")

    def symbol_stats(self) -> dict:
        """segment-decoder counters of the last decompress_shard call (fcx_dctx_symbol_stats):
        Huffman settle rounds, serial fallbacks (total and per sub-stream kind), Golomb rounds
        and fallbacks"""
        n = len(self.SYMBOL_STATS)
        vals = (ctypes.c_uint64 * n)()
        _check(lib().fcx_dctx_symbol_stats(self._h, vals, n), "fcx_dctx_symbol_stats")
        return dict(zip(self.SYMBOL_STATS, [int(v) for v in vals]))


def decompress_gpu(blob: bytes, cap: int = None, device: int = 0, ctx: "DContext" = None) -> bytes:
    """whole FCX7 file -> bytes with the GPU decoder (cap defaults to the header's total,
    which wraps mod 2^32: pass cap for larger files)"""
    own = ctx is None
    if own:
        ctx = DContext(device)
    try:
        return ctx.decompress_host(blob, cap)
    finally:
        if own:
            ctx.close()


def decompress_range(blob: bytes, off: int, n: int, device: int = 0) -> bytes:
    """decoded bytes [off, off + n) of a whole FCX7 or FCX8 file with the GPU decoder: only the
    records the range touches are expanded"""
    ctx = DContext(device)
    try:
        return ctx.decompress_range_host(blob, off, n)
    finally:
        ctx.close()


def verify(blob: bytes, data: bytes, block_bytes: int = BLOCK_BYTES, device: int = 0):
    """does the FCX7 or FCX8 file `blob` decode back to `data`, block by block?  Returns (stats, differing
    blocks) as DContext.verify_stream; it does when stats["differ"] == 0 and stats["bytes"] == 0"""
    import io

    ctx = DContext(device)
    try:
        return ctx.verify_stream(io.BytesIO(blob), io.BytesIO(data), block_bytes, max(0, len(blob) - HEADER_BYTES))
    finally:
        ctx.close()


def repair(blob: bytes, data: bytes, block_bytes: int = BLOCK_BYTES, device: int = 0) -> bytes:
    """the repair sidecar (an FCXR file) of the FCX7 or FCX8 file `blob`, made from `data` in blocks of
    block_bytes: with it, decompress_repaired(blob, ...) returns `data` exactly"""
    ctx = DContext(device)
    try:
        return ctx.repair_build_host(blob, data, block_bytes)
    finally:
        ctx.close()


def decompress_repaired(blob: bytes, repair: bytes, device: int = 0) -> bytes:
    """the FCX7 or FCX8 file `blob` decoded and mended by its FCXR file: the bytes that were compressed"""
    ctx = DContext(device)
    try:
        return ctx.repair_apply_host(blob, repair)
    finally:
        ctx.close()


def crc32(data: bytes, crc: int = 0) -> int:
    """the host mirror of the device digest: zlib.crc32(data, crc)"""
    return int(lib().fcx_crc32(crc, data, len(data)))


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """the CRC-32 of A + B from those of A and B and len(B)"""
    return int(lib().fcx_crc32_combine(crc_a, crc_b, len_b))


def digest(data: bytes, block_bytes: int = BLOCK_BYTES, device: int = 0) -> bytes:
    """the content digest (an FCXD file) of `data` in blocks of block_bytes: the CRC-32 of every block and of the
    whole, computed on the GPU; with it check(blob, ...) tests a compressed file without `data`"""
    ctx = DContext(device)
    try:
        return ctx.digest_host(data, block_bytes)
    finally:
        ctx.close()


def check(blob: bytes, digest: bytes, repair: bytes = None, device: int = 0):
    """does the FCX7 or FCX8 file `blob`, mended by its FCXR file when one is given, still give the bytes the FCXD
    file `digest` was made from?  Returns (stats, failing blocks) as DContext.check_stream; it does when
    stats["differ"] == 0 and stats["bytes"] == 0"""
    ctx = DContext(device)
    try:
        return ctx.check_host(blob, digest, repair)
    finally:
        ctx.close()


def find(blob: bytes, pattern: bytes, max_hits: int = None, device: int = 0):
    """where `pattern` (1 to 256 bytes) occurs in what the FCX7 or FCX8 file `blob` decodes to: (count,
    [offsets]) as DContext.find; the file is decoded and searched on the GPU, only the offsets come back"""
    ctx = DContext(device)
    try:
        return ctx.find(blob, pattern, max_hits)
    finally:
        ctx.close()


class PatternSet:
    """up to 64 byte patterns of 1 to 256 bytes (4096 in all) compiled for the set calls (fcx_pattern_set_create);
    ignore_case folds A to Z, and nothing else, in patterns and text"""
    FOLD_ASCII = 1

    def __init__(self, patterns, ignore_case: bool = False, flags: int = None):
        pats = [bytes(p) for p in patterns]
        lens = (ctypes.c_uint32 * max(len(pats), 1))(*[len(p) for p in pats])
        h = ctypes.c_void_p()
        self._h = None
        _check(lib().fcx_pattern_set_create(ctypes.byref(h), b"".join(pats) or b"\0", lens, len(pats),
                                            (self.FOLD_ASCII if ignore_case else 0) if flags is None else flags),
               "fcx_pattern_set_create")
        self._h = h
        self._n = len(pats)

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return self._n

    def info(self) -> dict:
        v = [ctypes.c_uint32(0) for _ in range(4)]
        _check(lib().fcx_pattern_set_info(self._h, *[ctypes.byref(x) for x in v]), "fcx_pattern_set_info")
        return dict(zip(("npat", "min_len", "max_len", "flags"), [int(x.value) for x in v]))

    def close(self):
        if self._h:
            lib().fcx_pattern_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def find_any(blob: bytes, patterns, ignore_case: bool = False, max_hits: int = None, device: int = 0):
    """(hits, counts): the offsets of what `blob` (FCX7 or FCX8) decodes to at which at least one of `patterns` occurs,
    ascending and each once (the first max_hits when given), and per pattern the number of positions at which it
    occurs; one scan on the GPU whatever the number of patterns"""
    ps = PatternSet(patterns, ignore_case)
    try:
        _n, hits, counts = _with_dctx(device, lambda c: c.find_set(blob, ps, max_hits))
        return hits, counts
    finally:
        ps.close()


def grep_any(blob: bytes, patterns, delim=b"\n", ignore_case: bool = False, device: int = 0) -> bytes:
    """the lines of what `blob` decodes to that hold at least one of `patterns`, each once, in order: grep -F -f (-i)"""
    ps = PatternSet(patterns, ignore_case)
    try:
        return _with_dctx(device, lambda c: c.grep_set_host(blob, ps, delim)[1])
    finally:
        ps.close()


def grep_any_ranges(blob: bytes, patterns, delim=b"\n", ignore_case: bool = False, device: int = 0):
    """(stats, [(start, end)], counts) of the lines grep_any() returns, through the stream form"""
    import io

    ps = PatternSet(patterns, ignore_case)
    try:
        return _with_dctx(device, lambda c: c.grep_set_stream(io.BytesIO(blob), ps, delim, max(0, len(blob) - HEADER_BYTES)))
    finally:
        ps.close()


def grep_context(blob: bytes, patterns, delim=b"\n", ignore_case: bool = False, invert: bool = False, before: int = 0, after: int = 0,
                 device: int = 0) -> bytes:
    """grep -F -f (-i) (-v) -B before -A after over what `blob` decodes to: the bytes of the selected lines, in order,
    without the `--` lines between blocks (grep_context_blocks() says where the blocks are)"""
    ps = PatternSet(patterns, ignore_case)
    try:
        return _with_dctx(device, lambda c: c.grep_blocks_host(blob, ps, delim, invert, before, after)[1])
    finally:
        ps.close()


def grep_context_blocks(blob: bytes, patterns, delim=b"\n", ignore_case: bool = False, invert: bool = False, before: int = 0,
                        after: int = 0, device: int = 0):
    """(stats, [(start, end, line, nlines)], counts) of the blocks whose bytes grep_context() returns, through the stream
    form"""
    import io

    ps = PatternSet(patterns, ignore_case)
    try:
        return _with_dctx(device, lambda c: c.grep_blocks_stream(io.BytesIO(blob), ps, delim, invert, before, after,
                                                                 max(0, len(blob) - HEADER_BYTES)))
    finally:
        ps.close()


class Regex:
    """a POSIX ERE subset over bytes compiled into a DFA of at most 64 states for the regex calls (fcx_regex_create; the
    syntax and the refusals: include/fcx.h).  `delim` is fixed here, since `.` and negated sets exclude it; ignore_case
    lets the letters of literals and sets match both ASCII cases"""
    FOLD_ASCII = 1
    MAX_PATTERN = 1024
    MAX_STATES = 64

    def __init__(self, expr: bytes, delim=0x0A, ignore_case: bool = False, flags: int = None):
        expr = bytes(expr)
        if isinstance(delim, (bytes, bytearray)):
            if len(delim) != 1:
                raise ValueError("delim is one byte")
            delim = delim[0]
        h = ctypes.c_void_p()
        self._h = None
        _check(lib().fcx_regex_create(ctypes.byref(h), expr or b"\0", len(expr), delim,
                                      (self.FOLD_ASCII if ignore_case else 0) if flags is None else flags), "fcx_regex_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        v = [ctypes.c_uint32(0) for _ in range(3)]
        d = ctypes.c_uint8(0)
        _check(lib().fcx_regex_info(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(d)), "fcx_regex_info")
        return dict(zip(("states", "classes", "flags", "delim"), [int(x.value) for x in v] + [int(d.value)]))

    def close(self):
        if self._h:
            lib().fcx_regex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grep_regex(blob: bytes, expr: bytes, delim=b"\n", ignore_case: bool = False, invert: bool = False, before: int = 0, after: int = 0,
               device: int = 0) -> bytes:
    """grep -E (-i) (-v) -B before -A after over what `blob` decodes to: the bytes of the selected lines, in order, without
    the `--` lines between blocks (grep_regex_blocks() says where the blocks are)"""
    rx = Regex(expr, delim, ignore_case)
    try:
        return _with_dctx(device, lambda c: c.grep_regex_blocks_host(blob, rx, invert, before, after)[1])
    finally:
        rx.close()


def grep_regex_blocks(blob: bytes, expr: bytes, delim=b"\n", ignore_case: bool = False, invert: bool = False, before: int = 0,
                      after: int = 0, device: int = 0):
    """(stats, [(start, end, line, nlines)]) of the blocks whose bytes grep_regex() returns, through the stream form"""
    import io

    rx = Regex(expr, delim, ignore_case)
    try:
        return _with_dctx(device, lambda c: c.grep_regex_blocks_stream(io.BytesIO(blob), rx, invert, before, after,
                                                                       max(0, len(blob) - HEADER_BYTES)))
    finally:
        rx.close()


class Cut:
    """GNU cut's LIST compiled for the cut calls (fcx_cut_create): fields=LIST with a one-byte separator, or
    byte_list=LIST; complement negates the selection.  The rule, the LIST syntax and the two differences from GNU cut
    (a line without a separator and with field 1 unselected gives an empty line; nothing is added behind an
    unterminated tail): include/fcx.h"""
    FIELDS = 1
    BYTES = 2
    COMPLEMENT = 1
    MAX_COLUMN = 4096

    def __init__(self, fields=None, byte_list=None, sep=b"\t", delim=b"\n", complement: bool = False):
        if (fields is None) == (byte_list is None):
            raise ValueError("give one of fields and byte_list")
        one = lambda b, what: b if isinstance(b, int) and 0 <= b <= 255 else (b[0] if len(b) == 1 else _one_byte(what))
        lst = fields if fields is not None else byte_list
        lst = lst.encode() if isinstance(lst, str) else bytes(lst)
        h = ctypes.c_void_p()
        self._h = None
        _check(lib().fcx_cut_create(ctypes.byref(h), lst, len(lst), self.FIELDS if fields is not None else self.BYTES,
                                    one(sep, "the separator"), one(delim, "the delimiter"), self.COMPLEMENT if complement else 0),
               "fcx_cut_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        v = [ctypes.c_uint32(0) for _ in range(4)]
        b = [ctypes.c_uint8(0) for _ in range(2)]
        _check(lib().fcx_cut_info(self._h, ctypes.byref(v[0]), ctypes.byref(b[0]), ctypes.byref(b[1]), ctypes.byref(v[1]),
                                  ctypes.byref(v[2]), ctypes.byref(v[3])), "fcx_cut_info")
        return {"mode": int(v[0].value), "sep": int(b[0].value), "delim": int(b[1].value), "flags": int(v[1].value),
                "mn": int(v[2].value), "open_end": bool(v[3].value)}

    def close(self):
        if self._h:
            lib().fcx_cut_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _one_byte(what):
    raise ValueError(what + " is one byte")


def _cut(blob, fields, byte_list, sep, delim, complement, ranges, device, size_only):
    ct = Cut(fields, byte_list, sep, delim, complement)
    try:
        if ranges is None:
            return _with_dctx(device, lambda c: c.cut_host(blob, ct, size_only))
        return _with_dctx(device, lambda c: c.cut_ranges_host(blob, ranges, ct, size_only))
    finally:
        ct.close()


def cut(blob: bytes, fields=None, byte_list=None, sep=b"\t", delim=b"\n", complement: bool = False, ranges=None, device: int = 0) -> bytes:
    """cut -f fields -d sep, or cut -b byte_list, (--complement) over what the FCX7 or FCX8 file `blob` decodes to, or over
    the ascending, disjoint (start, end) ranges of it (a grep's lines or blocks): decoded and cut on the GPU, only the
    cut bytes come back.  Without ranges the file is decoded twice (the size first: DContext.cut_host)"""
    return _cut(blob, fields, byte_list, sep, delim, complement, ranges, device, False)[2]


def cut_size(blob: bytes, fields=None, byte_list=None, sep=b"\t", delim=b"\n", complement: bool = False, ranges=None, device: int = 0) -> int:
    """the number of bytes cut() would return; nothing is gathered"""
    return _cut(blob, fields, byte_list, sep, delim, complement, ranges, device, True)[0]


def _with_dctx(device, fn):
    ctx = DContext(device)
    try:
        return fn(ctx)
    finally:
        ctx.close()


def count_lines(blob: bytes, delim=b"\n", device: int = 0) -> dict:
    """the lines of what the FCX7 or FCX8 file `blob` decodes to, counted on the GPU: {delimiters, lines, decoded,
    tail_bytes}; an unterminated tail is a line"""
    return _with_dctx(device, lambda c: c.count_lines(blob, delim))


def decompress_lines(blob: bytes, first: int, count: int = None, delim=b"\n", device: int = 0) -> bytes:
    """lines [first, first + count) (0-based; count None: to the end) of what `blob` decodes to, each with its
    delimiter: only the records that hold them are expanded"""
    return _with_dctx(device, lambda c: c.decompress_lines(blob, first, count, delim))


def line_numbers(blob: bytes, offsets, delim=b"\n", device: int = 0):
    """the line (0-based) on which each of the ascending decoded offsets lies"""
    return _with_dctx(device, lambda c: c.line_numbers(blob, offsets, delim))


def find_lines(blob: bytes, pattern: bytes, delim=b"\n", device: int = 0):
    """[(offset, line)] of every occurrence of `pattern` in what `blob` decodes to: find(), then the line of each
    hit in a second pass (lines 0-based)"""
    def both(c):
        _, hits = c.find(blob, pattern)
        return list(zip(hits, c.line_numbers(blob, hits, delim)))
    return _with_dctx(device, both)


def grep(blob: bytes, pattern: bytes, delim=b"\n", device: int = 0) -> bytes:
    """the lines of what the FCX7 or FCX8 file `blob` decodes to that hold `pattern` (1 to 256 bytes without the
    delimiter), each once and with its delimiter, in order: grep -F on the GPU, only the lines' bytes come back"""
    return _with_dctx(device, lambda c: c.grep_host(blob, pattern, delim)[1])


def grep_ranges(blob: bytes, pattern: bytes, delim=b"\n", device: int = 0):
    """(stats, [(start, end)]) of the lines of what `blob` decodes to that hold `pattern`: the byte ranges grep()
    prints, for decompress_ranges or a viewer; stats: {lines, bytes, hits, judged, decoded}"""
    import io

    return _with_dctx(device, lambda c: c.grep_stream(io.BytesIO(blob), pattern, delim, max(0, len(blob) - HEADER_BYTES)))


def my_compress_file_lz77(block: bytes) -> bytes:
    """one block (<= 1 MiB) -> payload, same bytes as my_compress_file_lz77 (:2115)"""
    n = len(block)
    out = ctypes.create_string_buffer(2 * n + 4096)
    got = lib().fcx_compress_block(block, n, out)
    if got == 0:
        raise FcxError(f"fcx_compress_block failed: {lib().fcx_last_error().decode(errors='replace')}")
    return out.raw[:got]


def my_decompress_file_lz77(payload: bytes, cap: int = BLOCK_BYTES + 8) -> bytes:
    """payload -> block bytes (reference decoder semantics, :2255)"""
    out = ctypes.create_string_buffer(cap)
    got = lib().fcx_decompress_block(payload, len(payload), out, cap)
    if got < 0:
        raise FcxError(f"fcx_decompress_block failed ({got})")
    return out.raw[:got]


def compress(data: bytes, block_bytes: int = BLOCK_BYTES, device: int = 0, ctx: "Context" = None) -> bytes:
    """whole FCX7 file for `data` (header + [u32 len][payload] per block)"""
    nblocks = (len(data) + block_bytes - 1) // block_bytes
    if not data:
        return write_header(0, 0)
    own = ctx is None
    if own:
        ctx = Context(device, block_bytes, min(len(data), 256 << 20))
    try:
        body = ctx.compress_host(data)
    finally:
        if own:
            ctx.close()
    return write_header(len(data), nblocks) + body


def decompress(blob: bytes) -> bytes:
    if len(blob) < HEADER_BYTES or blob[:3] != b"FCX" or blob[3:4] != b"7":
        raise FcxError("not an FCX7 (LZ77) stream")
    total, nblocks = struct.unpack_from("<IH", blob, 4)
    off, out = HEADER_BYTES, []
    for _ in range(nblocks):
        (sz,) = struct.unpack_from("<I", blob, off)
        off += 4
        out.append(my_decompress_file_lz77(blob[off:off + sz]))
        off += sz
    return b"".join(out)


# ---- -c lz78 (FCX8): my_compress_file_lz78 (my_compress.cpp:3127-3476) on the GPU ----
def lz78_bound(n: int, block_bytes: int = BLOCK_BYTES) -> int:
    """output capacity for compress_lz78: records are <= ~9.1 B per input byte + ~600 B"""
    nb = (n + block_bytes - 1) // block_bytes
    return HEADER_BYTES + 10 * n + 4096 * max(nb, 1)


def my_compress_file_lz78(block: bytes) -> bytes:
    """one block (<= 1 MiB) -> payload, same bytes as my_compress_file_lz78 (:3127)"""
    n = len(block)
    if n == 0:
        return b""
    out = ctypes.create_string_buffer(10 * n + 4096)
    got = lib().fcx_lz78_compress_block(block, n, out)
    if got == 0:
        raise FcxError(f"fcx_lz78_compress_block failed: {lib().fcx_last_error().decode(errors='replace')}")
    return out.raw[:got]


def compress_lz78(data: bytes, block_bytes: int = BLOCK_BYTES) -> bytes:
    """whole FCX8 file for `data` (main() with -c lz78, :4073-4136)"""
    cap = lz78_bound(len(data), block_bytes)
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64()
    try:
        _check(lib().fcx_lz78_compress_host(data, len(data), block_bytes, out, cap, ctypes.byref(n)),
               "fcx_lz78_compress_host")
    finally:
        lib().fcx_lz78_release()   # the codec caches ~40 B of device scratch per input byte
    return out.raw[:n.value]


def lz78_compress_shard(d_in: int, n: int, block_bytes: int, d_out: int, cap: int, stream: int = 0) -> int:
    """n device bytes at d_in -> FCX8 records (no header) at d_out; returns their byte count.  The
    scratch stays cached on the current device for the next call (lz78_release frees it)."""
    out = ctypes.c_uint64(0)
    _check(lib().fcx_lz78_compress_shard(ctypes.c_void_p(d_in), n, block_bytes, ctypes.c_void_p(d_out), cap,
                                         ctypes.byref(out), ctypes.c_void_p(stream)), "fcx_lz78_compress_shard")
    return out.value


def my_decompress_file_lz78(payload: bytes, cap: int = BLOCK_BYTES + 8) -> bytes:
    """one payload -> block bytes on the GPU (reference decoder semantics, :3478)"""
    out = ctypes.create_string_buffer(max(cap, 1))
    got = lib().fcx_lz78_decompress_block(payload, len(payload), out, cap)
    if got < 0:
        raise FcxError(f"fcx_lz78_decompress_block failed ({got}): {lib().fcx_last_error().decode(errors='replace')}")
    return out.raw[:got]


def decompress_lz78(blob: bytes, cap: int = None) -> bytes:
    """whole FCX8 file -> bytes on the GPU (main() decompress mode, :4137-4204)"""
    caps = [cap]
    if cap is None:   # the header's total (+ slack), then the per-block bound if the total wrapped
        total, nb = struct.unpack_from("<IH", blob, 4) if len(blob) >= HEADER_BYTES else (0, 0)
        caps = [total + 64 * nb + 64, nb * (BLOCK_BYTES + 8) + 1]
    for i, c in enumerate(caps):
        out = ctypes.create_string_buffer(max(c, 1))
        n = ctypes.c_uint64()
        rc = lib().fcx_lz78_decompress_host(blob, len(blob), out, c, ctypes.byref(n))
        if rc == -2 and i + 1 < len(caps):   # FCX_ERR_CAPACITY
            continue
        _check(rc, "fcx_lz78_decompress_host")
        return out.raw[:n.value]


def lz78_decode_batch_records() -> int:
    """records per internal batch of DContext.decompress_lz78_shard (its scratch is per batch)"""
    return int(lib().fcx_lz78_decode_batch_records())


def lz78_release() -> None:
    """frees the LZ78 compress scratch cached on the current HIP device"""
    _check(lib().fcx_lz78_release(), "fcx_lz78_release")


# ---- multi-GPU (fcx_dist_*: block ranges per GPU, RCCL concatenation) ----------------
DIST_GATHER, DIST_ALLGATHER = 0, 1


def dist_block_range(nblocks: int, rank: int, nranks: int, share0_ppm: int = 0):
    """the C partition (fcx_dist_block_range, or fcx_dist_block_range_w with a rank-0 share);
    equals my_compress_amd.dist.block_range"""
    b0, b1 = ctypes.c_uint64(), ctypes.c_uint64()
    if share0_ppm:
        lib().fcx_dist_block_range_w(nblocks, rank, nranks, share0_ppm, ctypes.byref(b0), ctypes.byref(b1))
    else:
        lib().fcx_dist_block_range(nblocks, rank, nranks, ctypes.byref(b0), ctypes.byref(b1))
    return b0.value, b1.value


def dist_gather_bound(n: int, block_bytes: int, nsub: int) -> int:
    """a peer's d_out capacity for Dist.compress_gather (pieces at their bound offsets)"""
    return int(lib().fcx_dist_gather_bound(n, block_bytes, nsub))


def dist_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(lib().fcx_dist_unique_id(buf), "fcx_dist_unique_id")
    return buf.raw


class Loop:
    """fcx_loop: the in-process loopback transport's hub (include/fcx.h).  Thread ranks on one
    device run the multi-rank protocols over it: Dist.loop(hub, r) per thread rank."""

    def __init__(self, nranks: int, device: int = 0, timeout_ms: int = 60000):
        self._h = ctypes.c_void_p()
        _check(lib().fcx_loop_create(ctypes.byref(self._h), nranks, device, timeout_ms), "fcx_loop_create")
        self.nranks = nranks

    def close(self):
        if self._h:
            lib().fcx_loop_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dist:
    """fcx_dist: communicator(s) of the multi-GPU compress path.
    Dist.local([0, 1, ...]) drives several devices from this process (the CLI's -g N);
    Dist.rank(n, r, uid, device) is one rank of a process-per-GPU job (RCCL);
    Dist.loop(hub, r) / Dist.loop_local(n, device) are the same forms over the loopback
    transport (thread ranks of one process on one device)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def local(cls, devices):
        h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices)
        _check(lib().fcx_dist_init_local(ctypes.byref(h), len(devices), arr), "fcx_dist_init_local")
        return cls(h)

    @classmethod
    def rank(cls, nranks: int, rank: int, uid: bytes, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().fcx_dist_init_rank(ctypes.byref(h), nranks, rank, uid, device), "fcx_dist_init_rank")
        return cls(h)

    @classmethod
    def loop(cls, hub: "Loop", rank: int):
        h = ctypes.c_void_p()
        _check(lib().fcx_dist_init_loop(ctypes.byref(h), hub._h, rank), "fcx_dist_init_loop")
        return cls(h)

    @classmethod
    def loop_local(cls, nranks: int, device: int = 0, timeout_ms: int = 60000):
        h = ctypes.c_void_p()
        _check(lib().fcx_dist_init_loop_local(ctypes.byref(h), nranks, device, timeout_ms), "fcx_dist_init_loop_local")
        return cls(h)

    def transport(self) -> str:
        return lib().fcx_dist_transport(self._h).decode()

    def debug_fail(self, piece: int):
        """testing: as a peer of compress_gather, treat sub-batch `piece` as failed (-1 = off)"""
        _check(lib().fcx_dist_debug_fail(self._h, piece), "fcx_dist_debug_fail")

    def gather_copy_ms(self) -> float:
        """rank 0 of the last compress_gather: device ms of its final moves of the peers' bytes
        behind its own segment (-1 on a peer)"""
        v = ctypes.c_float(-1.0)
        _check(lib().fcx_dist_gather_copy_ms(self._h, ctypes.byref(v)), "fcx_dist_gather_copy_ms")
        return float(v.value)

    def close(self):
        if self._h:
            lib().fcx_dist_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        n, loc = ctypes.c_int(), ctypes.c_int()
        _check(lib().fcx_dist_size(self._h, ctypes.byref(n), ctypes.byref(loc)), "fcx_dist_size")
        return n.value, loc.value

    def concat(self, d_seg: int, seg_len: int, d_out: int, cap: int, mode: int = DIST_GATHER, stream: int = 0) -> int:
        """this rank's device segment -> the concatenation in rank order at d_out; returns its length"""
        tot = ctypes.c_uint64()
        _check(lib().fcx_dist_concat(self._h, 0, ctypes.c_void_p(d_seg), seg_len, ctypes.c_void_p(d_out), cap,
                                     ctypes.byref(tot), mode, ctypes.c_void_p(stream)), "fcx_dist_concat")
        return tot.value

    def compress_gather(self, ctx: "Context", d_in: int, n: int, rank_bytes, nsub: int, d_out: int, cap: int,
                        stream: int = 0) -> int:
        """the strong-scaling step (fcx_dist_compress_gather): this rank compresses its n device
        bytes (peers: in nsub pieces, each sent to rank 0 when done) and rank 0 ends with every
        rank's records in block order at d_out; returns that length on rank 0, bytes sent elsewhere"""
        rb = (ctypes.c_uint64 * len(rank_bytes))(*rank_bytes)
        tot = ctypes.c_uint64()
        _check(lib().fcx_dist_compress_gather(self._h, ctx._h, ctypes.c_void_p(d_in), n, rb, nsub,
                                              ctypes.c_void_p(d_out), cap, ctypes.byref(tot),
                                              ctypes.c_void_p(stream)), "fcx_dist_compress_gather")
        return tot.value

    def compress_host(self, data: bytes, block_bytes: int = BLOCK_BYTES, round_bytes: int = 0) -> bytes:
        """records ([u32 len][payload]...) of data, block ranges over this process's devices"""
        cap = shard_bound(len(data), block_bytes)
        out = ctypes.create_string_buffer(max(cap, 1))
        got = ctypes.c_uint64()
        _check(lib().fcx_dist_compress_host(self._h, data, len(data), block_bytes, round_bytes, out, cap,
                                            ctypes.byref(got)), "fcx_dist_compress_host")
        return out.raw[:got.value]

