"""The line calls' entry points exist and check their arguments before they touch a device (include/fcx.h:
fcx_lines_index_shard, fcx_lines_locate_shard, fcx_decompress_lines_shard, fcx_lines_of_shard, their three
stream and three host forms, and fcx_dctx_lines_stats), and the binding exposes them.  Without a device a valid
file gets as far as the device and fails there with FCX_ERR_HIP: there is no silent host path behind the C ABI
(the command line's is its own, tests/test_lines_cli.py)."""
import ctypes

import lines_model as model
import my_compress_amd as mc
import oracle
from test_cli import gpu_present

FCX_ERR_ARG, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -3, -4
U64 = ctypes.c_uint64


def fake_ctx():
    """zeroed memory in the place of a context: its device index (0) is all that is read before the device
    is asked for, and an argument error comes before even that"""
    buf = ctypes.create_string_buffer(1 << 16)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def some_memory():
    rec = ctypes.create_string_buffer(256)
    return rec, ctypes.cast(rec, ctypes.c_void_p)


def test_lines_index_shard_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    rec, p = some_memory()
    stats = (U64 * 4)(7, 7, 7, 7)
    assert L.fcx_lines_index_shard(None, b"7", p, 64, 1, 10, None, stats, None) == FCX_ERR_ARG
    assert b"fcx_lines_index_shard" in L.fcx_last_error()
    assert L.fcx_lines_index_shard(ctx, b"7", p, 64, 1, 10, None, None, None) == FCX_ERR_ARG    # stats
    assert L.fcx_lines_index_shard(ctx, b"7", None, 64, 1, 10, None, stats, None) == FCX_ERR_ARG  # d_rec
    for kind in (b"9", b"\0", b"x"):
        assert L.fcx_lines_index_shard(ctx, kind, p, 64, 1, 10, None, stats, None) == FCX_ERR_ARG
        assert b"kind" in L.fcx_last_error()
    assert list(stats) == [7, 7, 7, 7]   # nothing was stored


def test_lines_locate_and_decompress_lines_shard_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    rec, p = some_memory()
    off, n = U64(7), U64(7)
    o, q = ctypes.byref(off), ctypes.byref(n)
    none3 = (None, None, None)
    assert L.fcx_lines_locate_shard(None, b"7", p, 64, 1, 10, *none3, 0, 1, o, q, None) == FCX_ERR_ARG
    assert b"fcx_lines_locate_shard" in L.fcx_last_error()
    assert L.fcx_lines_locate_shard(ctx, b"7", p, 64, 1, 10, *none3, 0, 1, None, q, None) == FCX_ERR_ARG
    assert L.fcx_lines_locate_shard(ctx, b"7", p, 64, 1, 10, *none3, 0, 1, o, None, None) == FCX_ERR_ARG
    assert L.fcx_lines_locate_shard(ctx, b"7", None, 64, 1, 10, *none3, 0, 1, o, q, None) == FCX_ERR_ARG
    assert L.fcx_lines_locate_shard(ctx, b"6", p, 64, 1, 10, *none3, 0, 1, o, q, None) == FCX_ERR_ARG
    assert L.fcx_decompress_lines_shard(None, b"7", p, 64, 1, 10, *none3, 0, 1, p, 8, q, None) == FCX_ERR_ARG
    assert b"fcx_decompress_lines_shard" in L.fcx_last_error()
    assert L.fcx_decompress_lines_shard(ctx, b"7", p, 64, 1, 10, *none3, 0, 1, p, 8, None, None) == FCX_ERR_ARG   # out_len
    assert L.fcx_decompress_lines_shard(ctx, b"7", p, 64, 1, 10, *none3, 0, 1, None, 8, q, None) == FCX_ERR_ARG   # d_out with cap
    assert L.fcx_decompress_lines_shard(ctx, b"7", None, 64, 1, 10, *none3, 0, 1, p, 8, q, None) == FCX_ERR_ARG
    assert L.fcx_decompress_lines_shard(ctx, b"x", p, 64, 1, 10, *none3, 0, 1, p, 8, q, None) == FCX_ERR_ARG
    # a part of an index: every way of giving one or two of the three arrays
    for mask in range(1, 7):
        part = tuple(p if mask >> i & 1 else None for i in range(3))
        assert L.fcx_lines_locate_shard(ctx, b"7", p, 64, 1, 10, *part, 0, 1, o, q, None) == FCX_ERR_ARG, mask
        assert b"index" in L.fcx_last_error()
        assert L.fcx_decompress_lines_shard(ctx, b"8", p, 64, 1, 10, *part, 0, 1, p, 8, q, None) == FCX_ERR_ARG, mask
        assert b"index" in L.fcx_last_error()
    assert (off.value, n.value) == (7, 7)


def test_lines_of_shard_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    rec, p = some_memory()
    assert L.fcx_lines_of_shard(None, b"7", p, 64, 1, 10, p, 2, p, None) == FCX_ERR_ARG
    assert b"fcx_lines_of_shard" in L.fcx_last_error()
    assert L.fcx_lines_of_shard(ctx, b"7", None, 64, 1, 10, p, 2, p, None) == FCX_ERR_ARG   # d_rec
    assert L.fcx_lines_of_shard(ctx, b"7", p, 64, 1, 10, None, 2, p, None) == FCX_ERR_ARG   # d_offsets
    assert L.fcx_lines_of_shard(ctx, b"7", p, 64, 1, 10, p, 2, None, None) == FCX_ERR_ARG   # d_lines
    assert L.fcx_lines_of_shard(ctx, b"9", p, 64, 1, 10, p, 2, p, None) == FCX_ERR_ARG
    assert L.fcx_dctx_lines_stats(None, None, 0) == FCX_ERR_ARG
    assert L.fcx_dctx_lines_stats(ctx, None, 5) == FCX_ERR_ARG
    assert b"fcx_dctx_lines_stats" in L.fcx_last_error()


def test_no_records_and_no_offsets_touch_no_device():
    L = mc.lib()
    if gpu_present():
        d = mc.DContext(0)
        try:
            assert d.lines_index_shard("7", 0, 0, 0) == dict(delimiters=0, lines=0, decoded=0, tail_bytes=0)
            assert d.lines_locate_shard("8", 0, 0, 0, 3, 5) == (0, 0)
            assert d.decompress_lines_shard("7", 0, 0, 0, 0, None, 0, 0) == 0
            d.lines_of_shard("7", 0, 0, 0, 0, 0, 0)
            assert d.lines_stats() == dict.fromkeys(mc.DContext.LINES_CALL_STATS, 0)
        finally:
            d.close()
        return
    keep, ctx = fake_ctx()   # (a context of zeros is enough: nothing of it is used but its counters, which are cleared)
    rec, p = some_memory()
    stats = (U64 * 4)(7, 7, 7, 7)
    assert L.fcx_lines_index_shard(ctx, b"7", None, 0, 0, 10, None, stats, None) == 0
    assert list(stats) == [0, 0, 0, 0]
    off, n = U64(7), U64(7)
    assert L.fcx_lines_locate_shard(ctx, b"8", None, 0, 0, 10, None, None, None, 3, 5, ctypes.byref(off), ctypes.byref(n), None) == 0
    assert (off.value, n.value) == (0, 0)
    n = U64(7)
    assert L.fcx_decompress_lines_shard(ctx, b"7", None, 0, 0, 10, None, None, None, 0, 2**64 - 1, None, 0, ctypes.byref(n), None) == 0
    assert n.value == 0
    assert L.fcx_lines_of_shard(ctx, b"7", p, 64, 1, 10, None, 0, None, None) == 0   # noff == 0: records or not
    assert L.fcx_lines_of_shard(ctx, b"8", None, 0, 0, 10, None, 0, None, None) == 0
    out = (U64 * 5)(7, 7, 7, 7, 7)
    assert L.fcx_dctx_lines_stats(ctx, out, 5) == 0 and list(out) == [0] * 5


def test_the_stream_and_host_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(model.text(7, 5000), 4096)
    stats = (U64 * 4)(7, 7, 7, 7)
    off, n = U64(7), U64(7)
    o, q = ctypes.byref(off), ctypes.byref(n)
    offs, lines = (U64 * 2)(1, 2), (U64 * 2)(7, 7)
    out = ctypes.create_string_buffer(64)
    no_read = ctypes.cast(None, mc.READ_FN)
    some_read = mc.READ_FN(lambda _u, _b, _c: -1)
    # fcx_lines_stream, fcx_lines_locate_stream, fcx_lines_of_stream
    assert L.fcx_lines_stream(None, some_read, None, 0, 10, stats) == FCX_ERR_ARG
    assert b"fcx_lines_stream" in L.fcx_last_error()
    assert L.fcx_lines_stream(ctx, no_read, None, 0, 10, stats) == FCX_ERR_ARG
    assert L.fcx_lines_stream(ctx, some_read, None, 0, 10, None) == FCX_ERR_ARG
    assert L.fcx_lines_locate_stream(None, some_read, None, 0, 10, 0, 1, o, q) == FCX_ERR_ARG
    assert b"fcx_lines_locate_stream" in L.fcx_last_error()
    assert L.fcx_lines_locate_stream(ctx, no_read, None, 0, 10, 0, 1, o, q) == FCX_ERR_ARG
    assert L.fcx_lines_locate_stream(ctx, some_read, None, 0, 10, 0, 1, None, q) == FCX_ERR_ARG
    assert L.fcx_lines_locate_stream(ctx, some_read, None, 0, 10, 0, 1, o, None) == FCX_ERR_ARG
    assert L.fcx_lines_of_stream(None, some_read, None, 0, 10, offs, 2, lines) == FCX_ERR_ARG
    assert b"fcx_lines_of_stream" in L.fcx_last_error()
    assert L.fcx_lines_of_stream(ctx, no_read, None, 0, 10, offs, 2, lines) == FCX_ERR_ARG
    assert L.fcx_lines_of_stream(ctx, some_read, None, 0, 10, None, 2, lines) == FCX_ERR_ARG
    assert L.fcx_lines_of_stream(ctx, some_read, None, 0, 10, offs, 2, None) == FCX_ERR_ARG
    down = (U64 * 3)(5, 9, 8)
    assert L.fcx_lines_of_stream(ctx, some_read, None, 0, 10, down, 3, (U64 * 3)()) == FCX_ERR_ARG   # a descending pair
    assert b"offset 2" in L.fcx_last_error()
    # fcx_lines_host, fcx_decompress_lines_host, fcx_lines_of_host
    assert L.fcx_lines_host(None, blob, len(blob), 10, stats) == FCX_ERR_ARG
    assert b"fcx_lines_host" in L.fcx_last_error()
    assert L.fcx_lines_host(ctx, None, len(blob), 10, stats) == FCX_ERR_ARG
    assert L.fcx_lines_host(ctx, blob, len(blob), 10, None) == FCX_ERR_ARG
    assert L.fcx_lines_host(ctx, b"NOTFCX" * 4, 24, 10, stats) == FCX_ERR_FORMAT
    assert L.fcx_decompress_lines_host(None, blob, len(blob), 10, 0, 1, out, 64, q) == FCX_ERR_ARG
    assert b"fcx_decompress_lines_host" in L.fcx_last_error()
    assert L.fcx_decompress_lines_host(ctx, None, len(blob), 10, 0, 1, out, 64, q) == FCX_ERR_ARG
    assert L.fcx_decompress_lines_host(ctx, blob, len(blob), 10, 0, 1, out, 64, None) == FCX_ERR_ARG
    assert L.fcx_decompress_lines_host(ctx, blob, len(blob), 10, 0, 1, None, 64, q) == FCX_ERR_ARG
    assert L.fcx_decompress_lines_host(ctx, b"NOTFCX" * 4, 24, 10, 0, 1, out, 64, q) == FCX_ERR_FORMAT
    assert L.fcx_lines_of_host(None, blob, len(blob), 10, offs, 2, lines) == FCX_ERR_ARG
    assert b"fcx_lines_of_host" in L.fcx_last_error()
    assert L.fcx_lines_of_host(ctx, None, len(blob), 10, offs, 2, lines) == FCX_ERR_ARG
    assert L.fcx_lines_of_host(ctx, blob, len(blob), 10, None, 2, lines) == FCX_ERR_ARG
    assert L.fcx_lines_of_host(ctx, blob, len(blob), 10, offs, 2, None) == FCX_ERR_ARG
    assert L.fcx_lines_of_host(ctx, b"NOTFCX" * 4, 24, 10, offs, 2, lines) == FCX_ERR_FORMAT
    assert list(stats) == [7, 7, 7, 7] and (off.value, n.value) == (7, 7) and list(lines) == [7, 7]


def test_a_valid_file_needs_the_device():
    L = mc.lib()
    data = model.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    if gpu_present():
        d = mc.DContext(0)
        try:
            st = d.count_lines(blob)
            assert [st[k] for k in mc.DContext.LINES_STATS] == model.stats(data, 0x0A)
            assert d.decompress_lines(blob, 1, 2) == b"".join(model.lines(data, 0x0A)[1:3])
            assert d.line_numbers(blob, [0, 4096, 5000]) == [model.nl(data, 0x0A, x) for x in (0, 4096, 5000)]
        finally:
            d.close()
        return
    keep, ctx = fake_ctx()
    stats = (U64 * 4)(7, 7, 7, 7)
    n = U64(7)
    assert L.fcx_lines_host(ctx, blob, len(blob), 10, stats) == FCX_ERR_HIP
    assert L.fcx_decompress_lines_host(ctx, blob, len(blob), 10, 0, 1, None, 0, ctypes.byref(n)) == FCX_ERR_HIP
    offs, lines = (U64 * 2)(1, 2), (U64 * 2)(7, 7)
    assert L.fcx_lines_of_host(ctx, blob, len(blob), 10, offs, 2, lines) == FCX_ERR_HIP
    assert list(stats) == [7, 7, 7, 7] and list(lines) == [7, 7]


def test_binding_exposes_the_line_calls():
    for name in ("lines_index_shard", "lines_locate_shard", "decompress_lines_shard", "lines_of_shard", "lines_stats",
                 "count_lines", "decompress_lines", "line_numbers"):
        assert callable(getattr(mc.DContext, name))
    for name in ("count_lines", "decompress_lines", "line_numbers", "find_lines"):
        assert callable(getattr(mc, name)) and name in mc.__all__
    assert len(mc.DContext.LINES_STATS) == 4 and len(mc.DContext.LINES_CALL_STATS) == 5
    L = mc.lib()
    for sym in ("fcx_lines_index_shard", "fcx_lines_locate_shard", "fcx_decompress_lines_shard", "fcx_lines_of_shard",
                "fcx_lines_stream", "fcx_lines_host", "fcx_lines_locate_stream", "fcx_decompress_lines_host",
                "fcx_lines_of_stream", "fcx_lines_of_host", "fcx_dctx_lines_stats"):
        assert hasattr(L, sym), sym
