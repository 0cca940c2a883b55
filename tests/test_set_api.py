"""The pattern set and its entry points exist and check their arguments before they touch a device (include/fcx.h:
fcx_pattern_set_*, fcx_find_set_*, fcx_grep_set_*, fcx_dctx_set_scan_stats), and the binding exposes them.  The set
is compiled on the host; without a device a valid file gets as far as the device and fails there with FCX_ERR_HIP."""
import ctypes

import pytest

import find_model as fm
import my_compress_amd as mc
import oracle
import set_model as sm
from test_cli import gpu_present
from test_find_api import fake_ctx

FCX_ERR_ARG, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -3, -4


def create(pats, flags=0):
    L = mc.lib()
    h = ctypes.c_void_p()
    lens = (ctypes.c_uint32 * max(len(pats), 1))(*[len(p) for p in pats])
    rc = L.fcx_pattern_set_create(ctypes.byref(h), b"".join(pats) or b"\0", lens, len(pats), flags)
    return rc, h


def test_create_checks_its_arguments():
    L = mc.lib()
    assert create([], 0)[0] == FCX_ERR_ARG and b"fcx_pattern_set_create" in L.fcx_last_error()
    assert create([b"a"] * 65)[0] == FCX_ERR_ARG and b"number of patterns" in L.fcx_last_error()
    rc, h = create([b"a"] * 64)
    assert rc == 0 and h.value
    L.fcx_pattern_set_destroy(h)
    lens = (ctypes.c_uint32 * 2)(1, 0)
    h = ctypes.c_void_p(7)
    assert L.fcx_pattern_set_create(ctypes.byref(h), b"ab", lens, 2, 0) == FCX_ERR_ARG and h.value is None   # a length of 0
    assert b"pattern length" in L.fcx_last_error()
    assert create([bytes(257)])[0] == FCX_ERR_ARG
    rc, h = create([bytes(256)])
    assert rc == 0
    L.fcx_pattern_set_destroy(h)
    assert create([bytes(256)] * 16 + [b"a"])[0] == FCX_ERR_ARG and b"FCX_SET_MAX_BYTES" in L.fcx_last_error()   # 4097 bytes
    rc, h = create([bytes(256)] * 16)
    assert rc == 0
    L.fcx_pattern_set_destroy(h)
    for flags in (2, 3, 0x80000000):
        assert create([b"ab"], flags)[0] == FCX_ERR_ARG and b"flag" in L.fcx_last_error()
    one = (ctypes.c_uint32 * 1)(2)
    assert L.fcx_pattern_set_create(None, b"ab", one, 1, 0) == FCX_ERR_ARG
    assert L.fcx_pattern_set_create(ctypes.byref(h), None, one, 1, 0) == FCX_ERR_ARG
    assert L.fcx_pattern_set_create(ctypes.byref(h), b"ab", None, 1, 0) == FCX_ERR_ARG
    L.fcx_pattern_set_destroy(None)   # as free(NULL)
    with pytest.raises(mc.FcxError):
        mc.PatternSet([])


def test_info_and_the_fold():
    ps = mc.PatternSet([b"QuErY", b"x", bytes(sm.FOLD_BYTES)], ignore_case=True)
    assert ps.info() == {"npat": 3, "min_len": 1, "max_len": 10, "flags": 1} and len(ps) == 3
    ps.close()
    ps = mc.PatternSet([b"ab", b"abc", b"ab"])   # a duplicate and a prefix are allowed
    assert ps.info() == {"npat": 3, "min_len": 2, "max_len": 3, "flags": 0}
    L = mc.lib()
    n = ctypes.c_uint32(9)
    assert L.fcx_pattern_set_info(ps.handle, ctypes.byref(n), None, None, None) == 0 and n.value == 3
    assert L.fcx_pattern_set_info(None, ctypes.byref(n), None, None, None) == FCX_ERR_ARG
    ps.close()
    # the fold of the definition: only A to Z
    assert sm.FOLD[0x41] == 0x61 and sm.FOLD[0x5A] == 0x7A and all(sm.FOLD[b] == b for b in (0x40, 0x5B, 0x60, 0x61, 0x7B, 0xC1, 0xE1))


def test_shard_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    arr = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    n = ctypes.c_uint64(7)
    st = (ctypes.c_uint64 * 5)(*[7] * 5)
    ps = mc.PatternSet([b"abc", b"x"])
    s = ps.handle
    f = L.fcx_find_set_shard
    assert f(None, b"7", p, 64, 1, s, None, 0, ctypes.byref(n), None, None) == FCX_ERR_ARG and b"fcx_find_set_shard" in L.fcx_last_error()
    assert f(ctx, b"7", p, 64, 1, None, None, 0, ctypes.byref(n), None, None) == FCX_ERR_ARG   # set
    assert f(ctx, b"7", p, 64, 1, s, None, 0, None, None, None) == FCX_ERR_ARG                  # nhits
    assert f(ctx, b"7", None, 64, 1, s, None, 0, ctypes.byref(n), None, None) == FCX_ERR_ARG    # d_rec
    assert f(ctx, b"7", p, 64, 1, s, None, 4, ctypes.byref(n), None, None) == FCX_ERR_ARG       # d_hits with cap
    for kind in (b"9", b"\0", b"x"):
        assert f(ctx, kind, p, 64, 1, s, None, 0, ctypes.byref(n), None, None) == FCX_ERR_ARG
    g = L.fcx_grep_set_shard
    assert g(None, b"7", p, 64, 1, 10, s, None, None, 0, st, None, None) == FCX_ERR_ARG and b"fcx_grep_set_shard" in L.fcx_last_error()
    assert g(ctx, b"7", p, 64, 1, 10, None, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert g(ctx, b"7", p, 64, 1, 10, s, None, None, 0, None, None, None) == FCX_ERR_ARG     # stats
    assert g(ctx, b"7", None, 64, 1, 10, s, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert g(ctx, b"7", p, 64, 1, 10, s, None, arr, 4, st, None, None) == FCX_ERR_ARG        # d_start with cap
    assert g(ctx, b"7", p, 64, 1, 10, s, arr, None, 4, st, None, None) == FCX_ERR_ARG        # d_end with cap
    assert g(ctx, b"5", p, 64, 1, 10, s, None, None, 0, st, None, None) == FCX_ERR_ARG
    assert g(ctx, b"7", p, 64, 1, ord("b"), s, None, None, 0, st, None, None) == FCX_ERR_ARG and b"holds the delimiter" in L.fcx_last_error()
    fold = mc.PatternSet([b"abc", b"x"], ignore_case=True)
    assert g(ctx, b"7", p, 64, 1, ord("B"), fold.handle, None, None, 0, st, None, None) == FCX_ERR_ARG and b"folded" in L.fcx_last_error()
    assert n.value == 7 and list(st) == [7] * 5
    assert L.fcx_dctx_set_scan_stats(None, None, 0) == FCX_ERR_ARG
    ps.close()
    fold.close()


def test_no_records_need_no_device():
    L = mc.lib()
    ps = mc.PatternSet([b"abc", b"x"])
    if gpu_present():
        d = mc.DContext(0)
        try:
            assert d.find_set_shard("7", 0, 0, 0, ps) == (0, [0, 0])
            assert d.grep_set_shard("8", 0, 0, 0, ps) == (dict.fromkeys(mc.DContext.GREP_STATS, 0), [0, 0])
            assert d.set_scan_stats() == dict.fromkeys(mc.DContext.SET_SCAN_STATS, 0)
        finally:
            d.close()
            ps.close()
        return
    keep, ctx = fake_ctx()
    n = ctypes.c_uint64(7)
    counts = (ctypes.c_uint64 * 2)(7, 7)
    st = (ctypes.c_uint64 * 5)(*[7] * 5)
    assert L.fcx_find_set_shard(ctx, b"7", None, 0, 0, ps.handle, None, 0, ctypes.byref(n), counts, None) == 0
    assert n.value == 0 and list(counts) == [0, 0]
    counts[0] = 7
    assert L.fcx_grep_set_shard(ctx, b"8", None, 0, 0, 10, ps.handle, None, None, 0, st, counts, None) == 0
    assert list(st) == [0] * 5 and list(counts) == [0, 0]
    sc = (ctypes.c_uint64 * 6)(*[7] * 6)
    assert L.fcx_dctx_set_scan_stats(ctx, sc, 6) == 0 and list(sc) == [0] * 6
    empty = mc.write_header(0, 0)
    out = ctypes.c_uint64(7)
    assert L.fcx_grep_set_host(ctx, empty, len(empty), 10, ps.handle, None, 0, ctypes.byref(out), st, counts) == 0 and out.value == 0
    ps.close()


def test_host_and_stream_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(fm.text(7, 5000), 4096)
    n = ctypes.c_uint64(7)
    out = ctypes.create_string_buffer(64)
    hits = (ctypes.c_uint64 * 8)()
    ps = mc.PatternSet([b"ab", b"q"])
    s = ps.handle
    ok = (ctx, blob, len(blob), s, hits, 8, ctypes.byref(n), None)
    for i in (0, 1, 3, 6):   # ctx, in, set, nhits
        args = list(ok)
        args[i] = None
        assert L.fcx_find_set_host(*args) == FCX_ERR_ARG and b"fcx_find_set_host" in L.fcx_last_error()
    assert L.fcx_find_set_host(ctx, blob, len(blob), s, None, 8, ctypes.byref(n), None) == FCX_ERR_ARG   # hits with cap
    assert L.fcx_find_set_host(ctx, b"NOTFCX" * 4, 24, s, hits, 8, ctypes.byref(n), None) == FCX_ERR_FORMAT
    ok = (ctx, blob, len(blob), 10, s, out, 64, ctypes.byref(n), None, None)
    for i in (0, 1, 4, 7):   # ctx, in, set, out_len
        args = list(ok)
        args[i] = None
        assert L.fcx_grep_set_host(*args) == FCX_ERR_ARG and b"fcx_grep_set_host" in L.fcx_last_error()
    assert L.fcx_grep_set_host(ctx, blob, len(blob), 10, s, None, 64, ctypes.byref(n), None, None) == FCX_ERR_ARG   # out with cap
    assert L.fcx_grep_set_host(ctx, blob, len(blob), ord("q"), s, out, 64, ctypes.byref(n), None, None) == FCX_ERR_ARG
    assert b"holds the delimiter" in L.fcx_last_error()
    assert L.fcx_grep_set_host(ctx, b"NOTFCX" * 4, 24, 10, s, out, 64, ctypes.byref(n), None, None) == FCX_ERR_FORMAT
    assert L.fcx_grep_set_host(ctx, blob[:-3], len(blob) - 3, 10, s, out, 64, ctypes.byref(n), None, None) == FCX_ERR_FORMAT
    no_read, no_hit, no_line = ctypes.cast(None, mc.READ_FN), ctypes.cast(None, mc.HIT_FN), ctypes.cast(None, mc.RANGE_FN)
    rd = mc.READ_FN(lambda _u, _b, _c: 0)
    assert L.fcx_find_set_stream(None, rd, None, 0, s, no_hit, None, None, None) == FCX_ERR_ARG and b"fcx_find_set_stream" in L.fcx_last_error()
    assert L.fcx_find_set_stream(ctx, no_read, None, 0, s, no_hit, None, None, None) == FCX_ERR_ARG
    assert L.fcx_find_set_stream(ctx, rd, None, 0, None, no_hit, None, None, None) == FCX_ERR_ARG
    assert L.fcx_find_set_stream(ctx, rd, None, 0, s, no_hit, None, None, None) == FCX_ERR_FORMAT   # (a reader at its end: no header)
    assert L.fcx_grep_set_stream(None, rd, None, 0, 10, s, no_line, None, None, None) == FCX_ERR_ARG and b"fcx_grep_set_stream" in L.fcx_last_error()
    assert L.fcx_grep_set_stream(ctx, no_read, None, 0, 10, s, no_line, None, None, None) == FCX_ERR_ARG
    assert L.fcx_grep_set_stream(ctx, rd, None, 0, 10, None, no_line, None, None, None) == FCX_ERR_ARG
    assert L.fcx_grep_set_stream(ctx, rd, None, 0, ord("a"), s, no_line, None, None, None) == FCX_ERR_ARG
    fold = mc.PatternSet([b"ab", b"q"], ignore_case=True)
    assert L.fcx_grep_set_stream(ctx, rd, None, 0, ord("Q"), fold.handle, no_line, None, None, None) == FCX_ERR_ARG
    assert L.fcx_grep_set_stream(ctx, rd, None, 0, 10, s, no_line, None, None, None) == FCX_ERR_FORMAT
    assert n.value == 7
    ps.close()
    fold.close()


def test_host_forms_on_a_valid_file_need_the_device():
    L = mc.lib()
    data = fm.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    pats = [data[100:104], data[200:201].upper()]
    if gpu_present():
        hits, counts = mc.find_any(blob, pats, ignore_case=True)
        assert hits == sm.hits_any(data, pats, True) and counts == sm.counts(data, pats, True)
        return
    keep, ctx = fake_ctx()
    ps = mc.PatternSet(pats, ignore_case=True)
    n = ctypes.c_uint64(7)
    assert L.fcx_find_set_host(ctx, blob, len(blob), ps.handle, None, 0, ctypes.byref(n), None) == FCX_ERR_HIP
    assert L.fcx_grep_set_host(ctx, blob, len(blob), 0, ps.handle, None, 0, ctypes.byref(n), None, None) == FCX_ERR_HIP
    ps.close()


def test_binding_exposes_the_sets():
    for name in ("find_set_shard", "grep_set_shard", "find_set", "grep_set_host", "grep_set_stream", "find_set_stream", "set_scan_stats"):
        assert callable(getattr(mc.DContext, name))
    for name in ("PatternSet", "find_any", "grep_any", "grep_any_ranges"):
        assert callable(getattr(mc, name)) and name in mc.__all__
    assert len(mc.DContext.SET_SCAN_STATS) == 6
