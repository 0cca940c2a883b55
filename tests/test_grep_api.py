"""The grep's and the multi-range decode's entry points exist and check their arguments before they touch a device
(include/fcx.h: fcx_grep_shard, fcx_decompress_ranges_shard, fcx_grep_host, fcx_decompress_ranges_host), and the
binding exposes them.  Without a device a valid file gets as far as the device and fails there with FCX_ERR_HIP:
there is no silent host path behind the C ABI."""
import ctypes

import find_model as fm
import grep_model as model
import my_compress_amd as mc
import oracle
from test_cli import gpu_present
from test_find_api import fake_ctx

FCX_ERR_ARG, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -3, -4


def test_grep_shard_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    rec = ctypes.create_string_buffer(64)
    p = ctypes.cast(rec, ctypes.c_void_p)
    arr = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    st = (ctypes.c_uint64 * 5)(*[7] * 5)
    pat = b"abc"
    assert L.fcx_grep_shard(None, b"7", p, 64, 1, 10, pat, 3, None, None, 0, st, None) == FCX_ERR_ARG
    assert b"fcx_grep_shard" in L.fcx_last_error()
    assert L.fcx_grep_shard(ctx, b"7", p, 64, 1, 10, None, 3, None, None, 0, st, None) == FCX_ERR_ARG     # pattern
    assert L.fcx_grep_shard(ctx, b"7", p, 64, 1, 10, pat, 3, None, None, 0, None, None) == FCX_ERR_ARG    # stats
    assert L.fcx_grep_shard(ctx, b"7", None, 64, 1, 10, pat, 3, None, None, 0, st, None) == FCX_ERR_ARG   # d_rec
    assert L.fcx_grep_shard(ctx, b"7", p, 64, 1, 10, pat, 3, None, arr, 4, st, None) == FCX_ERR_ARG       # d_start with cap
    assert L.fcx_grep_shard(ctx, b"7", p, 64, 1, 10, pat, 3, arr, None, 4, st, None) == FCX_ERR_ARG       # d_end with cap
    for kind in (b"9", b"\0", b"x"):
        assert L.fcx_grep_shard(ctx, kind, p, 64, 1, 10, pat, 3, None, None, 0, st, None) == FCX_ERR_ARG
    for plen in (0, 257, 300, 0xFFFFFFFF):
        assert L.fcx_grep_shard(ctx, b"8", p, 64, 1, 10, bytes(300), plen, None, None, 0, st, None) == FCX_ERR_ARG
        assert b"pattern length" in L.fcx_last_error()
    for pat, d in ((b"a\nb", 10), (b"\n", 10), (b"ab\0", 0), (bytes(255) + b"\xFF", 0xFF)):
        assert L.fcx_grep_shard(ctx, b"7", p, 64, 1, d, pat, len(pat), None, None, 0, st, None) == FCX_ERR_ARG
        assert b"holds the delimiter" in L.fcx_last_error()
    assert list(st) == [7] * 5   # nothing was stored


def test_ranges_shard_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    a = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    n = ctypes.c_uint64(7)
    ok = (ctx, b"7", p, 64, 1, None, None, a, a, 2, a, 16, ctypes.byref(n), None)

    def call(**kw):
        names = ["ctx", "kind", "rec", "len", "nb", "ro", "do", "s", "e", "nr", "out", "cap", "n", "st"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.fcx_decompress_ranges_shard(*args)

    assert call(ctx=None) == FCX_ERR_ARG and b"fcx_decompress_ranges_shard" in L.fcx_last_error()
    assert call(n=None) == FCX_ERR_ARG
    assert call(rec=None) == FCX_ERR_ARG
    assert call(s=None) == FCX_ERR_ARG and call(e=None) == FCX_ERR_ARG
    assert call(out=None) == FCX_ERR_ARG
    assert call(ro=a) == FCX_ERR_ARG and b"half an index" in L.fcx_last_error()
    assert call(do=a) == FCX_ERR_ARG
    for kind in (b"9", b"\0"):
        assert call(kind=kind) == FCX_ERR_ARG
    assert n.value == 7
    assert L.fcx_dctx_ranges_stats(None, None, 0) == FCX_ERR_ARG
    assert L.fcx_dctx_grep_scratch(None, None) == FCX_ERR_ARG


def test_no_records_and_no_ranges_need_no_device():
    L = mc.lib()
    if gpu_present():
        d = mc.DContext(0)
        try:
            assert d.grep_shard("7", 0, 0, 0, b"abc") == dict.fromkeys(mc.DContext.GREP_STATS, 0)
            assert d.decompress_ranges_shard("7", 0, 0, 0, 0, 0, 0, 0, 0) == 0
        finally:
            d.close()
        return
    keep, ctx = fake_ctx()
    st = (ctypes.c_uint64 * 5)(*[7] * 5)
    # (a context of zeros is enough: nothing of it is used but its counters, which are cleared)
    assert L.fcx_grep_shard(ctx, b"7", None, 0, 0, 10, b"abc", 3, None, None, 0, st, None) == 0
    assert list(st) == [0] * 5
    n = ctypes.c_uint64(7)
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert L.fcx_decompress_ranges_shard(ctx, b"8", p, 64, 1, None, None, None, None, 0, None, 0, ctypes.byref(n), None) == 0
    assert n.value == 0
    blob = oracle.compress_file(fm.text(7, 5000), 4096)
    assert L.fcx_decompress_ranges_host(ctx, blob, len(blob), None, None, 0, None, 0, ctypes.byref(n)) == 0
    empty = mc.write_header(0, 0)
    out = ctypes.c_uint64(7)
    assert L.fcx_grep_host(ctx, empty, len(empty), 10, b"ab", 2, None, 0, ctypes.byref(out), st) == 0
    assert out.value == 0 and list(st) == [0] * 5


def test_host_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(fm.text(7, 5000), 4096)
    n = ctypes.c_uint64(7)
    out = ctypes.create_string_buffer(64)
    ok = (ctx, blob, len(blob), 10, b"ab", 2, out, 64, ctypes.byref(n), None)
    for i in (0, 1, 4, 8):   # ctx, in, pattern, out_len
        args = list(ok)
        args[i] = None
        assert L.fcx_grep_host(*args) == FCX_ERR_ARG and b"fcx_grep_host" in L.fcx_last_error()
    assert L.fcx_grep_host(ctx, blob, len(blob), 10, b"ab", 2, None, 64, ctypes.byref(n), None) == FCX_ERR_ARG   # out with cap
    for plen in (0, 257):
        assert L.fcx_grep_host(ctx, blob, len(blob), 10, bytes(300), plen, out, 64, ctypes.byref(n), None) == FCX_ERR_ARG
    assert L.fcx_grep_host(ctx, blob, len(blob), 10, b"a\nb", 3, out, 64, ctypes.byref(n), None) == FCX_ERR_ARG
    assert b"holds the delimiter" in L.fcx_last_error()
    assert L.fcx_grep_host(ctx, b"NOTFCX" * 4, 24, 10, b"ab", 2, out, 64, ctypes.byref(n), None) == FCX_ERR_FORMAT
    assert L.fcx_grep_host(ctx, blob[:-3], len(blob) - 3, 10, b"ab", 2, out, 64, ctypes.byref(n), None) == FCX_ERR_FORMAT
    r = (ctypes.c_uint64 * 2)(0, 5)
    assert L.fcx_decompress_ranges_host(None, blob, len(blob), r, r, 2, out, 64, ctypes.byref(n)) == FCX_ERR_ARG
    assert b"fcx_decompress_ranges_host" in L.fcx_last_error()
    assert L.fcx_decompress_ranges_host(ctx, None, len(blob), r, r, 2, out, 64, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_host(ctx, blob, len(blob), None, r, 2, out, 64, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_host(ctx, blob, len(blob), r, None, 2, out, 64, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_host(ctx, blob, len(blob), r, r, 2, None, 64, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_host(ctx, blob, len(blob), r, r, 2, out, 64, None) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_host(ctx, b"NOTFCX" * 4, 24, r, r, 2, out, 64, ctypes.byref(n)) == FCX_ERR_FORMAT
    assert n.value == 7


def test_host_forms_on_a_valid_file_need_the_device():
    L = mc.lib()
    data = fm.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    pat = data[100:104]
    assert 10 not in pat
    want = model.selected(data, pat, 10)
    if gpu_present():
        d = mc.DContext(0)
        try:
            assert d.grep_host(blob, pat)[1] == model.join(data, want)
            assert d.decompress_ranges_host(blob, want) == model.join(data, want)
        finally:
            d.close()
        return
    keep, ctx = fake_ctx()
    n = ctypes.c_uint64(7)
    assert L.fcx_grep_host(ctx, blob, len(blob), 10, pat, len(pat), None, 0, ctypes.byref(n), None) == FCX_ERR_HIP
    r = (ctypes.c_uint64 * 2)(0, 5)
    out = ctypes.create_string_buffer(64)
    assert L.fcx_decompress_ranges_host(ctx, blob, len(blob), r, r, 1, out, 64, ctypes.byref(n)) == FCX_ERR_HIP


def test_binding_exposes_the_grep():
    for name in ("grep_shard", "decompress_ranges_shard", "grep_host", "decompress_ranges_host", "ranges_stats", "grep_scratch"):
        assert callable(getattr(mc.DContext, name))
    assert callable(mc.grep) and "grep" in mc.__all__
    assert len(mc.DContext.GREP_STATS) == 5 and len(mc.DContext.RANGES_STATS) == 5


def test_stream_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    no_read, no_write, no_line = ctypes.cast(None, mc.READ_FN), ctypes.cast(None, mc.WRITE_FN), ctypes.cast(None, mc.RANGE_FN)
    rd = mc.READ_FN(lambda _u, _b, _c: 0)
    wr = mc.WRITE_FN(lambda _u, _b, _n: 0)
    assert L.fcx_grep_stream(None, rd, None, 0, 10, b"ab", 2, no_line, None, None) == FCX_ERR_ARG
    assert b"fcx_grep_stream" in L.fcx_last_error()
    assert L.fcx_grep_stream(ctx, no_read, None, 0, 10, b"ab", 2, no_line, None, None) == FCX_ERR_ARG
    assert L.fcx_grep_stream(ctx, rd, None, 0, 10, None, 2, no_line, None, None) == FCX_ERR_ARG
    for plen in (0, 257):
        assert L.fcx_grep_stream(ctx, rd, None, 0, 10, bytes(300), plen, no_line, None, None) == FCX_ERR_ARG
    assert L.fcx_grep_stream(ctx, rd, None, 0, 0x41, b"bAc".upper(), 3, no_line, None, None) == FCX_ERR_ARG
    assert b"holds the delimiter" in L.fcx_last_error()
    assert L.fcx_grep_stream(ctx, rd, None, 0, 10, b"ab", 2, no_line, None, None) == FCX_ERR_FORMAT   # (a reader at its end: no header)
    s, e = (ctypes.c_uint64 * 3)(0, 100, 50), (ctypes.c_uint64 * 3)(5, 200, 60)
    n = ctypes.c_uint64(7)
    assert L.fcx_decompress_ranges_stream(None, rd, wr, None, 0, s, e, 3, ctypes.byref(n)) == FCX_ERR_ARG
    assert b"fcx_decompress_ranges_stream" in L.fcx_last_error()
    assert L.fcx_decompress_ranges_stream(ctx, no_read, wr, None, 0, s, e, 3, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_stream(ctx, rd, no_write, None, 0, s, e, 3, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_stream(ctx, rd, wr, None, 0, None, e, 3, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_decompress_ranges_stream(ctx, rd, wr, None, 0, s, None, 3, ctypes.byref(n)) == FCX_ERR_ARG
    # the order is checked on the host, before anything is read: descending, overlapping, end < start
    assert L.fcx_decompress_ranges_stream(ctx, rd, wr, None, 0, s, e, 3, ctypes.byref(n)) == FCX_ERR_ARG
    assert b"range 2 " in L.fcx_last_error()
    s2, e2 = (ctypes.c_uint64 * 2)(0, 4), (ctypes.c_uint64 * 2)(5, 9)
    assert L.fcx_decompress_ranges_stream(ctx, rd, wr, None, 0, s2, e2, 2, ctypes.byref(n)) == FCX_ERR_ARG and b"range 1 " in L.fcx_last_error()
    s3, e3 = (ctypes.c_uint64 * 2)(0, 9), (ctypes.c_uint64 * 2)(5, 8)
    assert L.fcx_decompress_ranges_stream(ctx, rd, wr, None, 0, s3, e3, 2, ctypes.byref(n)) == FCX_ERR_ARG and b"range 1 " in L.fcx_last_error()
    assert n.value == 7
    assert L.fcx_decompress_ranges_stream(ctx, rd, wr, None, 0, None, None, 0, ctypes.byref(n)) == 0 and n.value == 0   # no ranges: nothing is read
    for name in ("grep_stream", "decompress_ranges_stream"):
        assert callable(getattr(mc.DContext, name))
    assert callable(mc.grep_ranges) and "grep_ranges" in mc.__all__
