"""The regex object and its entry points exist and check their arguments before they touch a device (include/fcx.h:
fcx_regex_*, fcx_grep_regex_blocks_shard / _stream / _host, fcx_dctx_regex_scan_stats), and the binding exposes them.
The expression is compiled on the host: what the compiler accepts and refuses is what regex_model accepts and refuses.
Without a device a valid file gets as far as the device and fails there with FCX_ERR_HIP."""
import ctypes
import re

import pytest

import find_model as fm
import my_compress_amd as mc
import oracle
import regex_model as rm
from test_cli import gpu_present
from test_find_api import fake_ctx
from test_regex_model import BOTH, POSIX, REFUSED

FCX_ERR_ARG, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -3, -4


def opts(flags=0, before=0, after=0):
    return ctypes.byref(mc.GrepOpts(flags, before, after))


def create(expr: bytes, d=0x0A, flags=0):
    h = ctypes.c_void_p(7)
    rc = mc.lib().fcx_regex_create(ctypes.byref(h), expr or b"\0", len(expr), d, flags)
    return rc, h


@pytest.mark.parametrize("fold", [0, 1])
def test_the_compiler_accepts_what_the_model_accepts(fold):
    for expr in BOTH + POSIX:
        rm.Nfa(expr, 0x0A, bool(fold))
        rx = mc.Regex(expr, 0x0A, bool(fold))
        info = rx.info()
        assert 2 <= info["states"] <= 64 and 2 <= info["classes"] <= 256 and info["flags"] == fold and info["delim"] == 0x0A, (expr, info)
        rx.close()


def test_the_compiler_refuses_what_the_model_refuses():
    L = mc.lib()
    for expr in REFUSED:
        rc, h = create(expr)
        assert rc == FCX_ERR_ARG and h.value is None, expr
        msg = L.fcx_last_error()
        sized = any(w in msg for w in (b"positions", b"states", b"empty string"))   # (no single offset is to blame)
        assert msg.startswith(b"fcx_regex_create: ") and (sized or re.search(rb" at offset \d+$", msg)), (expr, msg)
    for expr, off in ((b"ab\\bcd", 2), (b"abc(^d)", 4), (b"ab|", 3), (b"a(b\nc)", 3), (b"ab{2,1}", 2), (b"abc[z-a]", 4)):
        assert create(expr)[0] == FCX_ERR_ARG and L.fcx_last_error().endswith(b" at offset %d" % off), (expr, L.fcx_last_error())


def test_the_delimiter_and_the_fold():
    L = mc.lib()
    assert create(b"a", 0x41)[0] == 0
    assert create(b"a", 0x41, 1)[0] == FCX_ERR_ARG and b"delimiter" in L.fcx_last_error()
    assert create(b"xAy", 0x61, 1)[0] == FCX_ERR_ARG
    assert create(b"[a-c]", 0x42, 1)[0] == FCX_ERR_ARG and create(b"[a-c]", 0x42)[0] == 0
    assert create(b"[A-C]", 0x42)[0] == FCX_ERR_ARG
    for expr, d in ((b"[^a-c]x", 0x42), (b"[[:upper:]]", 0x42), (b"\\w", 0x5F), (b"\\s\\S", 0x0A), (b".", 0x00), (b"\\W", 0x21)):
        rc, h = create(expr, d, 1)
        assert rc == 0, (expr, L.fcx_last_error())
        L.fcx_regex_destroy(h)
    assert create(b"[[:upper:]]", 0x42, 0)[0] == 0
    for flags in (2, 3, 0x80000000):
        assert create(b"ab", 0x0A, flags)[0] == FCX_ERR_ARG and b"flag" in L.fcx_last_error()


def test_the_limits():
    L = mc.lib()
    assert create(b"")[0] == FCX_ERR_ARG and b"FCX_REGEX_MAX_PATTERN" in L.fcx_last_error()
    assert create(b"a" * 1025)[0] == FCX_ERR_ARG
    for expr, states in ((b"^a{61}b", 64), (b"^[^#]{61}#", 64), (b"a[^b]{4}b", 33), (b"#", 2), (b"^#", 3)):
        rx = mc.Regex(expr)
        assert rx.info()["states"] == states, expr
        rx.close()
    for expr in (b"^a{62}b", b"^[^#]{62}#", b"a[^b]{5}b"):
        assert create(expr)[0] == FCX_ERR_ARG and b"more than 64 states" in L.fcx_last_error(), expr
    assert create(b"a.{20}b")[0] == FCX_ERR_ARG and b"4096 states" in L.fcx_last_error()
    assert create(b"(a{4}){16}{16}")[0] == FCX_ERR_ARG and b"64 states" in L.fcx_last_error()   # 1024 positions pass, 1026 states do not
    assert create(b"(a{4}){16}{16}a")[0] == FCX_ERR_ARG and b"1024 positions" in L.fcx_last_error()
    assert create(b"(a{255}){255}")[0] == FCX_ERR_ARG
    assert L.fcx_regex_create(None, b"ab", 2, 10, 0) == FCX_ERR_ARG
    h = ctypes.c_void_p(7)
    assert L.fcx_regex_create(ctypes.byref(h), None, 2, 10, 0) == FCX_ERR_ARG and h.value is None
    L.fcx_regex_destroy(None)   # as free(NULL)
    n = ctypes.c_uint32(9)
    assert L.fcx_regex_info(None, ctypes.byref(n), None, None, None) == FCX_ERR_ARG
    rx = mc.Regex(b"ab", b"\0", ignore_case=True)
    assert L.fcx_regex_info(rx.handle, ctypes.byref(n), None, None, None) == 0 and n.value == 3
    assert rx.info() == {"states": 3, "classes": 3, "flags": 1, "delim": 0}
    rx.close()
    with pytest.raises(mc.FcxError, match="offset 4$"):
        mc.Regex(b"a**|*")
    with pytest.raises(ValueError):
        mc.Regex(b"a", b"ab")


def test_the_shard_form_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    arr = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    st = (ctypes.c_uint64 * 8)(*[7] * 8)
    rx = mc.Regex(b"ab+c")
    r, g, o = rx.handle, L.fcx_grep_regex_blocks_shard, opts(1, 2, 3)
    assert g(None, b"7", p, 64, 1, r, o, None, None, None, 0, st, None) == FCX_ERR_ARG and b"fcx_grep_regex_blocks_shard" in L.fcx_last_error()
    assert g(ctx, b"7", p, 64, 1, None, o, None, None, None, 0, st, None) == FCX_ERR_ARG    # regex
    assert g(ctx, b"7", p, 64, 1, r, o, None, None, None, 0, None, None) == FCX_ERR_ARG     # stats
    assert g(ctx, b"7", None, 64, 1, r, o, None, None, None, 0, st, None) == FCX_ERR_ARG    # d_rec
    for missing in range(3):                                                                 # an array with cap
        a = [arr, arr, arr]
        a[missing] = None
        assert g(ctx, b"7", p, 64, 1, r, o, *a, 4, st, None) == FCX_ERR_ARG
    for kind in (b"9", b"\0", b"x"):
        assert g(ctx, kind, p, 64, 1, r, o, None, None, None, 0, st, None) == FCX_ERR_ARG and b"kind" in L.fcx_last_error()
    assert g(ctx, b"7", p, 64, 1, r, None, None, None, None, 0, st, None) == FCX_ERR_ARG and b"options" in L.fcx_last_error()
    for flags in (2, 3, 0x80000000):
        assert g(ctx, b"7", p, 64, 1, r, opts(flags), None, None, None, 0, st, None) == FCX_ERR_ARG and b"flag" in L.fcx_last_error()
    assert g(ctx, b"8", p, 64, 1, r, opts(0, 4097, 0), None, None, None, 0, st, None) == FCX_ERR_ARG
    assert b"FCX_GREP_MAX_CONTEXT" in L.fcx_last_error()
    assert g(ctx, b"8", p, 64, 1, r, opts(1, 0, 4097), None, None, None, 0, st, None) == FCX_ERR_ARG
    assert g(ctx, b"8", p, 64, 1, r, opts(0, 0xFFFFFFFF, 0), None, None, None, 0, st, None) == FCX_ERR_ARG
    zero = ctypes.cast(ctypes.create_string_buffer(1 << 15), ctypes.c_void_p)   # zeroed memory is not a regex
    assert g(ctx, b"7", p, 64, 1, zero, o, None, None, None, 0, st, None) == FCX_ERR_ARG and b"not a regex" in L.fcx_last_error()
    assert list(st) == [7] * 8
    assert L.fcx_dctx_regex_scan_stats(None, None, 0) == FCX_ERR_ARG
    assert L.fcx_dctx_regex_scan_stats(ctx, None, 4) == FCX_ERR_ARG and L.fcx_dctx_regex_scan_stats(ctx, st, -1) == FCX_ERR_ARG
    rx.close()


def test_no_records_need_no_device():
    L = mc.lib()
    rx = mc.Regex(b"ab+c")
    try:
        if gpu_present():
            d = mc.DContext(0)
            try:
                assert d.grep_regex_blocks_shard("8", 0, 0, 0, rx, invert=True, before=4096, after=1) == dict.fromkeys(mc.DContext.GREP_BLOCK_STATS, 0)
                assert d.grep_scratch() == 0 and d.regex_scan_stats() == dict.fromkeys(mc.DContext.REGEX_SCAN_STATS, 0)
            finally:
                d.close()
            return
        keep, ctx = fake_ctx()
        st = (ctypes.c_uint64 * 8)(*[7] * 8)
        assert L.fcx_grep_regex_blocks_shard(ctx, b"8", None, 0, 0, rx.handle, opts(1, 4096, 1), None, None, None, 0, st, None) == 0
        assert list(st) == [0] * 8
        sc = (ctypes.c_uint64 * 4)(*[7] * 4)
        assert L.fcx_dctx_regex_scan_stats(ctx, sc, 4) == 0 and list(sc) == [0] * 4
        v = ctypes.c_uint64(7)
        assert L.fcx_dctx_grep_scratch(ctx, ctypes.byref(v)) == 0 and v.value == 0
        empty = mc.write_header(0, 0)
        out = ctypes.c_uint64(7)
        st[0] = 7
        assert L.fcx_grep_regex_blocks_host(ctx, empty, len(empty), rx.handle, opts(1), None, 0, ctypes.byref(out), st) == 0
        assert out.value == 0 and list(st) == [0] * 8
    finally:
        rx.close()


def test_host_and_stream_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(fm.text(7, 5000), 4096)
    n = ctypes.c_uint64(7)
    out = ctypes.create_string_buffer(64)
    rx = mc.Regex(b"ab|q$")
    r, o = rx.handle, opts(1, 1, 1)
    ok = (ctx, blob, len(blob), r, o, out, 64, ctypes.byref(n), None)
    for i in (0, 1, 3, 4, 7):   # ctx, in, regex, opts, out_len
        args = list(ok)
        args[i] = None
        assert L.fcx_grep_regex_blocks_host(*args) == FCX_ERR_ARG and b"fcx_grep_regex_blocks_host" in L.fcx_last_error()
    assert L.fcx_grep_regex_blocks_host(ctx, blob, len(blob), r, o, None, 64, ctypes.byref(n), None) == FCX_ERR_ARG   # out with cap
    assert L.fcx_grep_regex_blocks_host(ctx, blob, len(blob), r, opts(0, 0, 5000), out, 64, ctypes.byref(n), None) == FCX_ERR_ARG
    assert L.fcx_grep_regex_blocks_host(ctx, blob, len(blob), r, opts(2), out, 64, ctypes.byref(n), None) == FCX_ERR_ARG
    assert L.fcx_grep_regex_blocks_host(ctx, b"NOTFCX" * 4, 24, r, o, out, 64, ctypes.byref(n), None) == FCX_ERR_FORMAT
    assert L.fcx_grep_regex_blocks_host(ctx, blob[:-3], len(blob) - 3, r, o, out, 64, ctypes.byref(n), None) == FCX_ERR_FORMAT
    no_read, no_block = ctypes.cast(None, mc.READ_FN), ctypes.cast(None, mc.BLOCK_FN)
    rd = mc.READ_FN(lambda _u, _b, _c: 0)
    f = L.fcx_grep_regex_blocks_stream
    assert f(None, rd, None, 0, r, o, no_block, None, None) == FCX_ERR_ARG and b"fcx_grep_regex_blocks_stream" in L.fcx_last_error()
    assert f(ctx, no_read, None, 0, r, o, no_block, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, None, o, no_block, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, r, None, no_block, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, r, opts(4), no_block, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, r, opts(0, 4097), no_block, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, None, 0, r, o, no_block, None, None) == FCX_ERR_FORMAT   # (a reader at its end: no header)
    assert n.value == 7
    rx.close()


def test_host_form_on_a_valid_file_needs_the_device():
    data = fm.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    expr = b"[a-z]+\\.$"
    if gpu_present():
        import context_model as cm

        want = cm.join(data, rm.blocks(data, rm.Nfa(expr), True, 1, 1))
        assert mc.grep_regex(blob, expr, invert=True, before=1, after=1) == want
        return
    keep, ctx = fake_ctx()
    rx = mc.Regex(expr)
    n = ctypes.c_uint64(7)
    assert mc.lib().fcx_grep_regex_blocks_host(ctx, blob, len(blob), rx.handle, opts(1, 1, 1), None, 0, ctypes.byref(n), None) == FCX_ERR_HIP
    rx.close()


def test_binding_exposes_the_regex_grep():
    for name in ("grep_regex_blocks_shard", "grep_regex_blocks_host", "grep_regex_blocks_stream", "regex_scan_stats"):
        assert callable(getattr(mc.DContext, name))
    assert mc.DContext.REGEX_SCAN_STATS == ("judged", "hits", "groups", "final_passes")
    for name in ("Regex", "grep_regex", "grep_regex_blocks"):
        assert callable(getattr(mc, name)) and name in mc.__all__
    assert (mc.Regex.MAX_PATTERN, mc.Regex.MAX_STATES, mc.Regex.FOLD_ASCII) == (1024, 64, 1)
