"""The device-resident FCX8 decoder's entry point exists and checks its arguments before it
touches a device (include/fcx.h: fcx_lz78_decompress_shard), and the binding exposes it."""
import ctypes

import my_compress_amd as mc

FCX_ERR_ARG = -1


def test_null_arguments_are_rejected_without_a_device():
    L = mc.lib()
    out_len = ctypes.c_uint64(7)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fake_ctx = ctypes.c_void_p(ctypes.addressof(buf))   # never dereferenced: a NULL comes first
    assert L.fcx_lz78_decompress_shard(None, p, 16, 1, p, 64, ctypes.byref(out_len), None) == FCX_ERR_ARG
    assert b"fcx_lz78_decompress_shard" in L.fcx_last_error()
    assert L.fcx_lz78_decompress_shard(fake_ctx, None, 16, 1, p, 64, ctypes.byref(out_len), None) == FCX_ERR_ARG
    assert L.fcx_lz78_decompress_shard(fake_ctx, p, 16, 1, None, 64, ctypes.byref(out_len), None) == FCX_ERR_ARG
    assert L.fcx_lz78_decompress_shard(fake_ctx, p, 16, 1, p, 64, None, None) == FCX_ERR_ARG


def test_binding_exposes_the_shard_call_and_the_batch_size():
    assert callable(getattr(mc.DContext, "decompress_lz78_shard"))
    assert mc.lz78_decode_batch_records() >= 1
