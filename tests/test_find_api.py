"""The search's entry points exist and check their arguments before they touch a device (include/fcx.h:
fcx_find_shard, fcx_find_host, fcx_find_stream), and the binding exposes them.  Without a device a valid
file gets as far as the device and fails there with FCX_ERR_HIP: there is no silent host search behind the
C ABI (the command line's host path is its own, tests/test_find_cli.py)."""
import ctypes

import find_model as model
import my_compress_amd as mc
import oracle
from test_cli import gpu_present

FCX_ERR_ARG, FCX_ERR_HIP, FCX_ERR_FORMAT = -1, -3, -4


def fake_ctx():
    """zeroed memory in the place of a context: its device index (0) is all that is read before the device
    is asked for, and an argument error comes before even that"""
    buf = ctypes.create_string_buffer(1 << 16)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_find_shard_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    rec = ctypes.create_string_buffer(64)
    p = ctypes.cast(rec, ctypes.c_void_p)
    n = ctypes.c_uint64(7)
    pat = b"abc"
    assert L.fcx_find_shard(None, b"7", p, 64, 1, pat, 3, None, 0, ctypes.byref(n), None) == FCX_ERR_ARG
    assert b"fcx_find_shard" in L.fcx_last_error()
    assert L.fcx_find_shard(ctx, b"7", p, 64, 1, None, 3, None, 0, ctypes.byref(n), None) == FCX_ERR_ARG   # pattern
    assert L.fcx_find_shard(ctx, b"7", p, 64, 1, pat, 3, None, 0, None, None) == FCX_ERR_ARG               # nhits
    assert L.fcx_find_shard(ctx, b"7", None, 64, 1, pat, 3, None, 0, ctypes.byref(n), None) == FCX_ERR_ARG  # d_rec
    assert L.fcx_find_shard(ctx, b"7", p, 64, 1, pat, 3, None, 4, ctypes.byref(n), None) == FCX_ERR_ARG    # d_hits with cap
    for kind in (b"9", b"\0", b"x"):
        assert L.fcx_find_shard(ctx, kind, p, 64, 1, pat, 3, None, 0, ctypes.byref(n), None) == FCX_ERR_ARG
    long = bytes(300)
    for plen in (0, 257, 300, 0xFFFFFFFF):
        assert L.fcx_find_shard(ctx, b"8", p, 64, 1, long, plen, None, 0, ctypes.byref(n), None) == FCX_ERR_ARG
        assert b"pattern length" in L.fcx_last_error()
    assert n.value == 7   # nothing was stored


def test_no_records_is_no_hits_and_no_device():
    L = mc.lib()
    if gpu_present():
        d = mc.DContext(0)
        try:
            assert d.find_shard("7", 0, 0, 0, b"abc") == 0
        finally:
            d.close()
        return
    keep, ctx = fake_ctx()
    n = ctypes.c_uint64(7)
    # (a context of zeros is enough: nothing of it is used but its counters, which are cleared)
    assert L.fcx_find_shard(ctx, b"7", None, 0, 0, b"abc", 3, None, 0, ctypes.byref(n), None) == 0
    assert n.value == 0


def test_find_host_rejects_bad_arguments_without_a_device():
    L = mc.lib()
    keep, ctx = fake_ctx()
    blob = oracle.compress_file(model.text(7, 5000), 4096)
    n = ctypes.c_uint64(7)
    out = (ctypes.c_uint64 * 4)()
    assert L.fcx_find_host(None, blob, len(blob), b"ab", 2, out, 4, ctypes.byref(n)) == FCX_ERR_ARG
    assert b"fcx_find_host" in L.fcx_last_error()
    assert L.fcx_find_host(ctx, None, len(blob), b"ab", 2, out, 4, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_find_host(ctx, blob, len(blob), None, 2, out, 4, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_find_host(ctx, blob, len(blob), b"ab", 2, out, 4, None) == FCX_ERR_ARG
    assert L.fcx_find_host(ctx, blob, len(blob), b"ab", 2, None, 4, ctypes.byref(n)) == FCX_ERR_ARG
    for plen in (0, 257):
        assert L.fcx_find_host(ctx, blob, len(blob), bytes(300), plen, out, 4, ctypes.byref(n)) == FCX_ERR_ARG
    assert L.fcx_find_host(ctx, b"NOTFCX" * 4, 24, b"ab", 2, out, 4, ctypes.byref(n)) == FCX_ERR_FORMAT
    no_read, no_hit = ctypes.cast(None, mc.READ_FN), ctypes.cast(None, mc.HIT_FN)
    assert L.fcx_find_stream(ctx, no_read, None, 0, b"ab", 2, no_hit, None, None) == FCX_ERR_ARG
    assert b"fcx_find_stream" in L.fcx_last_error()
    assert L.fcx_dctx_find_stats(None, None, 0) == FCX_ERR_ARG
    assert L.fcx_dctx_set_find_window(None, 5) == FCX_ERR_ARG
    assert n.value == 7


def test_find_host_on_a_valid_file_needs_the_device():
    L = mc.lib()
    data = model.text(7, 5000)
    blob = oracle.compress_file(data, 4096)
    pat = data[100:108]
    want = model.hits(data, pat)
    if gpu_present():
        d = mc.DContext(0)
        try:
            assert d.find(blob, pat) == (len(want), want)
        finally:
            d.close()
        return
    keep, ctx = fake_ctx()
    n = ctypes.c_uint64(7)
    assert L.fcx_find_host(ctx, blob, len(blob), pat, len(pat), None, 0, ctypes.byref(n)) == FCX_ERR_HIP
    assert n.value == 7


def test_binding_exposes_the_search():
    for name in ("find_shard", "find", "find_stats", "set_find_window"):
        assert callable(getattr(mc.DContext, name))
    assert callable(mc.find) and mc.FIND_MAX_PATTERN == 256
    assert len(mc.DContext.FIND_STATS) == 6
