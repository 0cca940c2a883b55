"""The context grep's entry points exist and check their arguments before they touch a device (include/fcx.h:
fcx_grep_blocks_shard / _stream / _host), and the binding exposes them.  Without a device a valid file gets as far as
the device and fails there with FCX_ERR_HIP."""
import ctypes

import context_model as cm
import find_model as fm
import my_compress_amd as mc
import oracle
from test_cli import gpu_present
from test_find_api import fake_ctx

FCX_ERR_ARG, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -3, -4


def opts(flags=0, before=0, after=0):
    return ctypes.byref(mc.GrepOpts(flags, before, after))


def test_the_shard_form_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    arr = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    st = (ctypes.c_uint64 * 8)(*[7] * 8)
    ps = mc.PatternSet([b"abc", b"x"])
    s, g, o = ps.handle, L.fcx_grep_blocks_shard, opts(1, 2, 3)
    assert g(None, b"7", p, 64, 1, 10, s, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG and b"fcx_grep_blocks_shard" in L.fcx_last_error()
    assert g(ctx, b"7", p, 64, 1, 10, None, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG    # set
    assert g(ctx, b"7", p, 64, 1, 10, s, o, None, None, None, 0, None, None, None) == FCX_ERR_ARG     # stats
    assert g(ctx, b"7", None, 64, 1, 10, s, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG    # d_rec
    for missing in range(3):                                                                           # an array with cap
        a = [arr, arr, arr]
        a[missing] = None
        assert g(ctx, b"7", p, 64, 1, 10, s, o, *a, 4, st, None, None) == FCX_ERR_ARG
    for kind in (b"9", b"\0", b"x"):
        assert g(ctx, kind, p, 64, 1, 10, s, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert g(ctx, b"7", p, 64, 1, 10, s, None, None, None, None, 0, st, None, None) == FCX_ERR_ARG and b"options" in L.fcx_last_error()
    for flags in (2, 3, 0x80000000):
        assert g(ctx, b"7", p, 64, 1, 10, s, opts(flags), None, None, None, 0, st, None, None) == FCX_ERR_ARG and b"flag" in L.fcx_last_error()
    assert g(ctx, b"8", p, 64, 1, 10, s, opts(0, 4097, 0), None, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert b"FCX_GREP_MAX_CONTEXT" in L.fcx_last_error()
    assert g(ctx, b"8", p, 64, 1, 10, s, opts(1, 0, 4097), None, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert g(ctx, b"8", p, 64, 1, 10, s, opts(0, 0xFFFFFFFF, 0), None, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert g(ctx, b"7", p, 64, 1, ord("b"), s, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG and b"holds the delimiter" in L.fcx_last_error()
    fold = mc.PatternSet([b"abc", b"x"], ignore_case=True)
    assert g(ctx, b"7", p, 64, 1, ord("B"), fold.handle, o, None, None, None, 0, st, None, None) == FCX_ERR_ARG and b"folded" in L.fcx_last_error()
    assert list(st) == [7] * 8
    ps.close()
    fold.close()


def test_no_records_need_no_device():
    L = mc.lib()
    ps = mc.PatternSet([b"abc", b"x"])
    try:
        if gpu_present():
            d = mc.DContext(0)
            try:
                assert d.grep_blocks_shard("8", 0, 0, 0, ps, invert=True, before=4096, after=1) == (dict.fromkeys(mc.DContext.GREP_BLOCK_STATS, 0), [0, 0])
                assert d.grep_scratch() == 0
            finally:
                d.close()
            return
        keep, ctx = fake_ctx()
        counts = (ctypes.c_uint64 * 2)(7, 7)
        st = (ctypes.c_uint64 * 8)(*[7] * 8)
        assert L.fcx_grep_blocks_shard(ctx, b"8", None, 0, 0, 10, ps.handle, opts(1, 4096, 1), None, None, None, 0, st, counts, None) == 0
        assert list(st) == [0] * 8 and list(counts) == [0, 0]
        v = ctypes.c_uint64(7)
        assert L.fcx_dctx_grep_scratch(ctx, ctypes.byref(v)) == 0 and v.value == 0
        empty = mc.write_header(0, 0)
        out = ctypes.c_uint64(7)
        st[0] = 7
        assert L.fcx_grep_blocks_host(ctx, empty, len(empty), 10, ps.handle, opts(1), None, 0, ctypes.byref(out), st, counts) == 0
        assert out.value == 0 and list(st) == [0] * 8
    finally:
        ps.close()


def test_host_and_stream_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(fm.text(7, 5000), 4096)
    n = ctypes.c_uint64(7)
    out = ctypes.create_string_buffer(64)
    ps = mc.PatternSet([b"ab", b"q"])
    s, o = ps.handle, opts(1, 1, 1)
    ok = (ctx, blob, len(blob), 10, s, o, out, 64, ctypes.byref(n), None, None)
    for i in (0, 1, 4, 5, 8):   # ctx, in, set, opts, out_len
        args = list(ok)
        args[i] = None
        assert L.fcx_grep_blocks_host(*args) == FCX_ERR_ARG and b"fcx_grep_blocks_host" in L.fcx_last_error()
    assert L.fcx_grep_blocks_host(ctx, blob, len(blob), 10, s, o, None, 64, ctypes.byref(n), None, None) == FCX_ERR_ARG   # out with cap
    assert L.fcx_grep_blocks_host(ctx, blob, len(blob), ord("q"), s, o, out, 64, ctypes.byref(n), None, None) == FCX_ERR_ARG
    assert L.fcx_grep_blocks_host(ctx, blob, len(blob), 10, s, opts(0, 0, 5000), out, 64, ctypes.byref(n), None, None) == FCX_ERR_ARG
    assert L.fcx_grep_blocks_host(ctx, b"NOTFCX" * 4, 24, 10, s, o, out, 64, ctypes.byref(n), None, None) == FCX_ERR_FORMAT
    assert L.fcx_grep_blocks_host(ctx, blob[:-3], len(blob) - 3, 10, s, o, out, 64, ctypes.byref(n), None, None) == FCX_ERR_FORMAT
    no_read, no_block = ctypes.cast(None, mc.READ_FN), ctypes.cast(None, mc.BLOCK_FN)
    rd = mc.READ_FN(lambda _u, _b, _c: 0)
    f = L.fcx_grep_blocks_stream
    assert f(None, rd, None, 0, 10, s, o, no_block, None, None, None) == FCX_ERR_ARG and b"fcx_grep_blocks_stream" in L.fcx_last_error()
    assert f(ctx, no_read, None, 0, 10, s, o, no_block, None, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, 10, None, o, no_block, None, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, 10, s, None, no_block, None, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, 10, s, opts(4), no_block, None, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, ord("a"), s, o, no_block, None, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, 10, s, o, no_block, None, None, None) == FCX_ERR_FORMAT   # (a reader at its end: no header)
    assert n.value == 7
    ps.close()


def test_host_form_on_a_valid_file_needs_the_device():
    data = fm.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    pats = [data[100:104]]
    if gpu_present():
        want = cm.join(data, cm.blocks(data, pats, 0x0A, invert=True, before=1, after=1))
        assert mc.grep_context(blob, pats, invert=True, before=1, after=1) == want
        return
    keep, ctx = fake_ctx()
    ps = mc.PatternSet(pats)
    n = ctypes.c_uint64(7)
    assert mc.lib().fcx_grep_blocks_host(ctx, blob, len(blob), 0, ps.handle, opts(1, 1, 1), None, 0, ctypes.byref(n), None, None) == FCX_ERR_HIP
    ps.close()


def test_binding_exposes_the_context_grep():
    for name in ("grep_blocks_shard", "grep_blocks_host", "grep_blocks_stream"):
        assert callable(getattr(mc.DContext, name))
    assert len(mc.DContext.GREP_BLOCK_STATS) == 8 and mc.DContext.GREP_INVERT == 1 and mc.DContext.GREP_MAX_CONTEXT == 4096
    for name in ("grep_context", "grep_context_blocks"):
        assert callable(getattr(mc, name)) and name in mc.__all__
    o = mc.GrepOpts(1, 2, 3)
    assert ctypes.sizeof(o) == 12 and (o.flags, o.before, o.after) == (1, 2, 3)
