"""Lifecycles of the contexts of the C ABI: scratch that is dropped and rebuilt when a call outgrows
it (fcx_ctx, and fcx_dctx across its FCX7 and FCX8 parts), the stage tables of the three profiled
paths, a context's state after a failed call, and the per-thread contexts of the block entry points.
Block size 4096 (one match tile); expected bytes from the oracle, as in test_gpu_parity.py."""
import math
import os
import subprocess
import sys

import pytest

import inputs
import my_compress_amd as mc
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 4096
STAGES = ["route", "match", "stitch", "emit", "hist", "tree", "block_layout", "scan_blocks", "zero", "encode",
          "headers"]
DSTAGES = ["tables", "symbols", "golomb", "lengths", "lz"]
D78STAGES = ["header", "index", "tables", "symbols", "links", "expand"]


def records(blob: bytes):
    """(records without the 10-byte file header, their count)"""
    return blob[10:], int.from_bytes(blob[8:10], "little")


def fcx7(data: bytes):
    """FCX7 records of data that the format gives back whole (the reference decoder's quirks, such
    as a one-symbol sub-stream decoding as zeros, do not touch it)"""
    blob = oracle.compress_file(data, BLOCK)
    assert oracle.decompress_file(blob, len(data) + 64) == data
    return records(blob)


def fcx8(data: bytes, block: int):
    """FCX8 records of text (no block ends in 0x00, so the format's tail-zero rule drops nothing)"""
    blob = oracle.lz78_compress_file(data, block)
    assert oracle.lz78_decompress_file(blob, len(data) + 64) == data
    return records(blob)


def compress(ctx, cuda, data: bytes, cap: int = None) -> bytes:
    """fcx_compress_shard on device-resident bytes: the records"""
    import torch

    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)
    d_out = torch.empty(mc.shard_bound(len(data), BLOCK), dtype=torch.uint8, device=cuda)
    n = ctx.compress_shard(d_in.data_ptr(), len(data), d_out.data_ptr(), d_out.numel() if cap is None else cap,
                           torch.cuda.current_stream().cuda_stream)
    return d_out[:n].cpu().numpy().tobytes()


def decode(dctx, cuda, recs_n, cap: int, lz78: bool = False) -> bytes:
    """fcx_decompress_shard / fcx_lz78_decompress_shard on device-resident records"""
    import torch

    recs, n = recs_n
    d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(cuda)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=cuda)
    fn = dctx.decompress_lz78_shard if lz78 else dctx.decompress_shard
    got = fn(d_in.data_ptr(), len(recs), n, d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    return d_out[:got].cpu().numpy().tobytes()


def check_stages(st, names):
    assert [n for n, _ in st] == names, st
    assert all(math.isfinite(ms) and ms >= 0 for _, ms in st), st


def test_compress_context_regrowth(cuda):
    """a context sized for one block: a three-block shard with a short tail drops and rebuilds the
    scratch; the calls before and after it see the same context"""
    ctx = mc.Context(0, BLOCK, BLOCK)
    try:
        for seed, n in ((21, 1000), (22, 2 * BLOCK + 1000), (23, 1000)):
            data = inputs.mosaic(seed, n)
            assert compress(ctx, cuda, data) == fcx7(data)[0], n
    finally:
        ctx.close()


def test_decoder_regrowth_both_formats(cuda):
    """one DContext: FCX7 shards of 1, 5 and 1 blocks (the per-block scratch grows once), between them
    FCX8 shards of 1 record and of 257 records of 64 B (past the 256-record batch: the second batch
    runs on the scratch of the first; the token scratch grows from the 1-record call's)"""
    d = mc.DContext(0)
    try:
        a, b, c = inputs.mosaic(31, 3000), inputs.mosaic(32, 4 * BLOCK + 777), inputs.mosaic(33, BLOCK)
        t1, t257 = inputs.generate("text", 34, 64), inputs.generate("text", 35, 257 * 64)
        assert decode(d, cuda, fcx7(a), len(a)) == a
        assert decode(d, cuda, fcx8(t1, 64), len(t1) + 64, lz78=True) == t1
        assert decode(d, cuda, fcx7(b), len(b)) == b
        r257 = fcx8(t257, 64)
        assert r257[1] == 257
        assert decode(d, cuda, r257, len(t257) + 64, lz78=True) == t257
        assert decode(d, cuda, fcx7(c), len(c)) == c
    finally:
        d.close()


def test_stage_tables(cuda):
    """the names and order of the three stage tables; which table a decoder context reports follows its
    last call; nothing is reported without profiling.  (The times are not compared to anything.)"""
    data = inputs.mosaic(43, 2 * BLOCK + 1000)
    text = inputs.generate("text", 42, 3 * 64)
    ctx, d = mc.Context(0, BLOCK, len(data)), mc.DContext(0)
    try:
        compress(ctx, cuda, data)
        assert ctx.stage_times() == []
        ctx.set_profiling(True)
        compress(ctx, cuda, data)
        check_stages(ctx.stage_times(), STAGES)
        ctx.set_profiling(False)
        compress(ctx, cuda, data)
        assert ctx.stage_times() == []

        r7, r8 = fcx7(data), fcx8(text, 64)
        assert decode(d, cuda, r7, len(data)) == data
        assert d.stage_times() == []
        d.set_profiling(True)
        assert decode(d, cuda, r7, len(data)) == data
        check_stages(d.stage_times(), DSTAGES)
        assert decode(d, cuda, r8, len(text) + 64, lz78=True) == text
        check_stages(d.stage_times(), D78STAGES)
        assert decode(d, cuda, r7, len(data)) == data
        check_stages(d.stage_times(), DSTAGES)
        d.set_profiling(False)
        assert decode(d, cuda, r8, len(text) + 64, lz78=True) == text
        assert d.stage_times() == []
        assert decode(d, cuda, r7, len(data)) == data
        assert d.stage_times() == []
    finally:
        ctx.close()
        d.close()


def test_context_survives_failed_call(cuda):
    """a call whose capacity is one byte short fails; the same context then does the call right"""
    data = inputs.mosaic(53, 2 * BLOCK + 1000)
    text = inputs.generate("text", 52, 5 * 64)
    want = fcx7(data)[0]
    ctx, d = mc.Context(0, BLOCK, len(data)), mc.DContext(0)
    try:
        with pytest.raises(mc.FcxError):
            compress(ctx, cuda, data, cap=len(want) - 1)
        assert compress(ctx, cuda, data, cap=len(want)) == want

        with pytest.raises(mc.FcxError):
            decode(d, cuda, fcx7(data), len(data) - 1)
        assert decode(d, cuda, fcx7(data), len(data)) == data

        with pytest.raises(mc.FcxError):
            decode(d, cuda, fcx8(text, 64), len(text) - 1, lz78=True)
        assert decode(d, cuda, fcx8(text, 64), len(text), lz78=True) == text
    finally:
        ctx.close()
        d.close()


_THREADS = r"""
import sys, threading
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import inputs, my_compress_amd as mc, oracle

data = inputs.mosaic(61, 3000)
text = inputs.generate("text", 62, 3000)
want = oracle.compress_block(data)
payload = oracle.lz78_compress_block(text)
assert oracle.lz78_decompress_block(payload, len(text) + 64) == text
bad = []

def both(who):
    if mc.my_compress_file_lz77(data) != want: bad.append(who + ": fcx_compress_block")
    if mc.my_decompress_file_lz78(payload) != text: bad.append(who + ": fcx_lz78_decompress_block")

t = threading.Thread(target=both, args=("thread",))
t.start()
t.join()
both("main")
both("main again")
assert not bad, bad
print("threads OK")
"""


def test_per_thread_owners(cuda):
    """fcx_compress_block and fcx_lz78_decompress_block keep a context per host thread: from a thread
    that exits (its contexts go with it), then from the main thread; the process ends cleanly"""
    p = subprocess.run([sys.executable, "-c", _THREADS, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "threads OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
