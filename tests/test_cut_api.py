"""The cut object and its entry points exist and check their arguments before they touch a device (include/fcx.h:
fcx_cut_*, fcx_dctx_cut_stats), and the binding exposes them.  LIST is compiled on the host: what the compiler accepts
and refuses, and the offset it names, is what cut_model's parser accepts, refuses and names.  Without a device a valid
file gets as far as the device and fails there with FCX_ERR_HIP."""
import ctypes

import pytest

import cut_model as km
import my_compress_amd as mc
import oracle
from test_cli import gpu_present
from test_find_api import fake_ctx

FCX_ERR_ARG, FCX_ERR_CAPACITY, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -2, -3, -4
ACCEPTED = ["1", "4096", "4097-", "-4096", "1-4096", "1,1,1", "7-7", "2,4", "3-", "-2", "2-3,5-", "1-"]
REFUSED = ["", "0", "1,0", "5-3", "4097", "1-4097", "4098-", "1,,2", "1,", ",1", "1 2", "a", "-", "1-2-3", "2-0", "1;2", "1-2,\n", "0-", "-0"]


def create(lst: bytes, mode=km.FIELDS, sep=0x2C, d=0x0A, flags=0):
    h = ctypes.c_void_p(7)
    rc = mc.lib().fcx_cut_create(ctypes.byref(h), lst, len(lst), mode, sep, d, flags)
    return rc, h


def test_the_compiler_accepts_what_the_model_accepts():
    for lst in ACCEPTED:
        for comp in (False, True):
            try:
                want = km.Sel(lst, comp)
            except km.ListError:
                assert lst == "1-" and comp
                assert create(lst.encode(), flags=1)[0] == FCX_ERR_ARG and b"offset 0" in mc.lib().fcx_last_error()
                continue
            for kw, mode in (({"fields": lst}, km.FIELDS), ({"byte_list": lst}, km.BYTES)):
                ct = mc.Cut(sep=b",", delim=b"\0", complement=comp, **kw)
                assert ct.info() == {"mode": mode, "sep": 0x2C if mode == km.FIELDS else 0, "delim": 0, "flags": int(comp), "mn": want.mn,
                                     "open_end": want.open_end}, (lst, comp)
                ct.close()


def test_the_compiler_refuses_what_the_model_refuses():
    L = mc.lib()
    for lst in REFUSED:
        with pytest.raises(km.ListError) as e:
            km.Sel(lst)
        for mode in (km.FIELDS, km.BYTES):
            rc, h = create(lst.encode(), mode)
            msg = L.fcx_last_error()
            assert rc == FCX_ERR_ARG and h.value is None, lst
            assert msg.startswith(b"fcx_cut_create: LIST offset %d: " % e.value.offset), (lst, msg)
    with pytest.raises(mc.FcxError, match="offset 2"):
        mc.Cut(fields="1,0")
    assert create(b"4096")[0] == 0 and create(b"4097")[0] == FCX_ERR_ARG and create(b"4097-")[0] == 0
    assert (mc.Cut.MAX_COLUMN, mc.Cut.FIELDS, mc.Cut.BYTES, mc.Cut.COMPLEMENT) == (4096, 1, 2, 1)


def test_the_other_arguments_of_create():
    L = mc.lib()
    assert create(b"1", sep=0x0A, d=0x0A)[0] == FCX_ERR_ARG and b"separator" in L.fcx_last_error()
    assert create(b"1", km.BYTES, sep=0x0A, d=0x0A)[0] == 0   # (bytes mode has no separator)
    for mode in (0, 3, 0x80000000):
        assert create(b"1", mode)[0] == FCX_ERR_ARG and b"mode" in L.fcx_last_error()
    for flags in (2, 3, 0x80000000):
        assert create(b"1", flags=flags)[0] == FCX_ERR_ARG and b"flag" in L.fcx_last_error()
    assert L.fcx_cut_create(None, b"1", 1, 1, 0x2C, 0x0A, 0) == FCX_ERR_ARG
    h = ctypes.c_void_p(7)
    assert L.fcx_cut_create(ctypes.byref(h), None, 1, 1, 0x2C, 0x0A, 0) == FCX_ERR_ARG and h.value is None
    L.fcx_cut_destroy(None)   # as free(NULL)
    assert L.fcx_cut_info(None, None, None, None, None, None, None) == FCX_ERR_ARG
    ct = mc.Cut(fields="2")
    mn = ctypes.c_uint32(0)
    assert L.fcx_cut_info(ct.handle, None, None, None, None, ctypes.byref(mn), None) == 0 and mn.value == 2
    ct.close()
    with pytest.raises(ValueError):
        mc.Cut(fields="1", byte_list="1")
    with pytest.raises(ValueError):
        mc.Cut()
    with pytest.raises(ValueError):
        mc.Cut(fields="1", sep=b"ab")


def test_the_device_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    o = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    n = ctypes.c_uint64(7)
    nn = ctypes.byref(n)
    st = (ctypes.c_uint64 * 6)(*[7] * 6)
    ct = mc.Cut(fields="2")
    k = ct.handle
    f = L.fcx_cut_shard
    assert f(None, b"7", p, 64, 1, k, o, 64, nn, st, None) == FCX_ERR_ARG and b"fcx_cut_shard" in L.fcx_last_error()
    assert f(ctx, b"7", p, 64, 1, None, o, 64, nn, st, None) == FCX_ERR_ARG     # cut
    assert f(ctx, b"7", p, 64, 1, k, o, 64, None, st, None) == FCX_ERR_ARG      # out_len
    assert f(ctx, b"7", None, 64, 1, k, o, 64, nn, st, None) == FCX_ERR_ARG     # d_rec with nblocks
    assert f(ctx, b"7", p, 64, 1, k, None, 64, nn, st, None) == FCX_ERR_ARG     # d_out with cap
    for kind in (b"9", b"\0", b"x"):
        assert f(ctx, kind, p, 64, 1, k, o, 64, nn, st, None) == FCX_ERR_ARG and b"kind" in L.fcx_last_error()
    f = L.fcx_cut_buffer
    assert f(None, p, 64, k, o, 64, nn, st, None) == FCX_ERR_ARG and b"fcx_cut_buffer" in L.fcx_last_error()
    assert f(ctx, p, 64, None, o, 64, nn, st, None) == FCX_ERR_ARG
    assert f(ctx, p, 64, k, o, 64, None, st, None) == FCX_ERR_ARG
    assert f(ctx, None, 64, k, o, 64, nn, st, None) == FCX_ERR_ARG
    assert f(ctx, p, 64, k, None, 64, nn, st, None) == FCX_ERR_ARG
    f = L.fcx_cut_ranges_shard
    ok = [ctx, b"8", p, 64, 1, None, None, p, p, 2, k, o, 64, nn, st, None]
    for i in (0, 2, 7, 8, 10, 11, 13):   # ctx, d_rec, d_start, d_end, cut, d_out, out_len
        a = list(ok)
        a[i] = None
        assert f(*a) == FCX_ERR_ARG and b"fcx_cut_ranges_shard" in L.fcx_last_error(), i
    a = list(ok)
    a[1] = b"6"
    assert f(*a) == FCX_ERR_ARG and b"kind" in L.fcx_last_error()
    for i in (5, 6):   # half an index
        a = list(ok)
        a[i] = p
        assert f(*a) == FCX_ERR_ARG and b"half an index" in L.fcx_last_error()
    assert n.value == 7 and list(st) == [7] * 6
    assert L.fcx_dctx_cut_stats(None, st, 6) == FCX_ERR_ARG and L.fcx_dctx_cut_stats(ctx, None, 6) == FCX_ERR_ARG
    assert L.fcx_dctx_cut_stats(ctx, st, -1) == FCX_ERR_ARG and L.fcx_dctx_cut_scratch(ctx, None) == FCX_ERR_ARG
    ct.close()


def test_nothing_to_cut_needs_no_device():
    L = mc.lib()
    ct = mc.Cut(byte_list="1-16", complement=True)
    try:
        if gpu_present():
            d = mc.DContext(0)
            try:
                zeros = dict.fromkeys(mc.DContext.CUT_STATS, 0)
                assert d.cut_shard("8", 0, 0, 0, ct) == (0, zeros) and d.cut_buffer(0, 0, ct) == (0, zeros)
                assert d.cut_ranges_shard("7", 0, 0, 0, 0, 0, 0, ct) == (0, zeros)
                assert d.cut_stats() == zeros and d.cut_scratch() == 0
            finally:
                d.close()
            return
        keep, ctx = fake_ctx()
        n = ctypes.c_uint64(7)
        st = (ctypes.c_uint64 * 6)(*[7] * 6)
        assert L.fcx_cut_shard(ctx, b"8", None, 0, 0, ct.handle, None, 0, ctypes.byref(n), st, None) == 0
        assert n.value == 0 and list(st) == [0] * 6
        n.value, st[0] = 7, 7
        assert L.fcx_cut_buffer(ctx, None, 0, ct.handle, None, 0, ctypes.byref(n), st, None) == 0 and n.value == 0 and list(st) == [0] * 6
        n.value, st[0] = 7, 7
        assert L.fcx_cut_ranges_shard(ctx, b"7", None, 0, 0, None, None, None, None, 0, ct.handle, None, 0, ctypes.byref(n), st, None) == 0
        assert n.value == 0 and list(st) == [0] * 6
        sc = (ctypes.c_uint64 * 6)(*[7] * 6)
        assert L.fcx_dctx_cut_stats(ctx, sc, 6) == 0 and list(sc) == [0] * 6
        v = ctypes.c_uint64(7)
        assert L.fcx_dctx_cut_scratch(ctx, ctypes.byref(v)) == 0 and v.value == 0
    finally:
        ct.close()


def test_host_and_stream_forms_reject_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(km.text(7, 5000), 4096)
    n = ctypes.c_uint64(7)
    nn = ctypes.byref(n)
    out = ctypes.create_string_buffer(64)
    ct = mc.Cut(fields="2", sep=b" ")
    k = ct.handle
    ok = (ctx, blob, len(blob), k, out, 64, nn, None)
    for i in (0, 1, 3, 4, 6):   # ctx, in, cut, out with cap, out_len
        a = list(ok)
        a[i] = None
        assert L.fcx_cut_host(*a) == FCX_ERR_ARG and b"fcx_cut_host" in L.fcx_last_error(), i
    assert L.fcx_cut_host(ctx, b"NOTFCX" * 4, 24, k, out, 64, nn, None) == FCX_ERR_FORMAT
    two = (ctypes.c_uint64 * 2)(0, 4)
    ok = (ctx, blob, len(blob), two, two, 2, k, out, 64, nn, None)
    for i in (0, 1, 3, 4, 6, 7, 9):   # ctx, in, starts, ends, cut, out with cap, out_len
        a = list(ok)
        a[i] = None
        assert L.fcx_cut_ranges_host(*a) == FCX_ERR_ARG and b"fcx_cut_ranges_host" in L.fcx_last_error(), i
    assert L.fcx_cut_ranges_host(ctx, blob[:-3], len(blob) - 3, two, two, 2, k, out, 64, nn, None) == FCX_ERR_FORMAT
    no_read, no_write = ctypes.cast(None, mc.READ_FN), ctypes.cast(None, mc.WRITE_FN)
    rd = mc.READ_FN(lambda _u, _b, _c: 0)
    f = L.fcx_cut_stream
    assert f(None, rd, no_write, None, 0, k, None) == FCX_ERR_ARG and b"fcx_cut_stream" in L.fcx_last_error()
    assert f(ctx, no_read, no_write, None, 0, k, None) == FCX_ERR_ARG
    assert f(ctx, rd, no_write, None, 0, None, None) == FCX_ERR_ARG
    assert f(ctx, rd, no_write, None, 0, k, None) == FCX_ERR_FORMAT   # (a reader at its end: no header)
    ct.close()


def test_host_form_on_a_valid_file_needs_the_device():
    data = km.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    if gpu_present():
        mode, sel = km.make_sel(fields="2-3")
        want = km.cut_np(data, sel, mode, 0x20, 0x0A)[0]
        assert mc.cut(blob, fields="2-3", sep=b" ") == want and mc.cut_size(blob, fields="2-3", sep=b" ") == len(want)
        return
    keep, ctx = fake_ctx()
    ct = mc.Cut(fields="2-3", sep=b" ")
    n = ctypes.c_uint64(7)
    assert mc.lib().fcx_cut_host(ctx, blob, len(blob), ct.handle, None, 0, ctypes.byref(n), None) == FCX_ERR_HIP
    ct.close()


def test_binding_exposes_the_cut():
    for name in ("cut_buffer", "cut_shard", "cut_ranges_shard", "cut_stream", "cut_host", "cut_ranges_host", "cut_stats", "cut_scratch"):
        assert callable(getattr(mc.DContext, name))
    assert mc.DContext.CUT_STATS == ("out_bytes", "judged", "delimiters", "separators", "separators_kept", "groups")
    for name in ("Cut", "cut", "cut_size"):
        assert callable(getattr(mc, name)) and name in mc.__all__
