"""The sparse unit's repeat filter and equal-key search (fcx_match.hip under FCX_SPARSE,
fcx_sparse_filter.h) against the oracle: seeded random bytes with chunks copied from p - d to p, at
the lengths, distances and positions where the search can go wrong (tile starts and halos, block
starts and ends, the window's far edge at 2047 / 2048, the 12-byte compare's boundary, the length
cap), with the sparse unit forced (mode 7) and routed (mode 0).  Bar: the bytes equal the oracle's.
"""
import ctypes
import random

import numpy as np
import pytest

import inputs
import my_compress_amd as mc
import oracle
from match_craft import geometry, plant, planted_input

pytestmark = pytest.mark.gpu

TILE, HALO = 4096, 2048
LENGTHS = (3, 4, 11, 12, 13, 257, 258, 259, 300)
DISTANCES = (1, 2, 3, 2046, 2047, 2048, 2049)
BLOCKS = (65536, 12293, 5000)


def model_max_flagged(L, data: bytes, block: int):
    """largest flagged count of any tile window (host model, position order) and the cap"""
    arr = np.frombuffer(data, dtype=np.uint8)
    out = (ctypes.c_uint32 * 4)()
    worst = 0
    for bs, be in geometry(len(data), block)[0]:
        for t0 in range(bs, be, TILE):
            lo, hi = max(bs, t0 - HALO), min(t0 + TILE, be - 2)
            if hi > lo:
                assert L.fcx_debug_sparse_filter(ctypes.c_void_p(arr.ctypes.data + lo), hi - lo, None, out) == 0
                worst = max(worst, out[0])
    return worst, out[1]


@pytest.fixture(scope="module")
def L():
    lib = mc.lib()
    lib.fcx_debug_sparse_filter.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_uint32)]
    return lib


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(block: int, cap_bytes: int):
        key = (block, cap_bytes)
        if key not in made:
            made[key] = mc.Context(0, block, cap_bytes)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _compress(ctx, cuda, data: bytes, block: int) -> bytes:
    import torch

    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)
    cap = mc.shard_bound(len(data), block)
    d_out = torch.empty(cap, dtype=torch.uint8, device=cuda)
    n = ctx.compress_shard(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    return mc.write_header(len(data), (len(data) + block - 1) // block) + d_out[:n].cpu().numpy().tobytes()


def check_both_modes(ctx, cuda, data: bytes, block: int, below_cap: bool, what):
    want = oracle.compress_file(data, block)
    ctx.set_match_mode(7)   # the sparse unit forced
    try:
        assert _compress(ctx, cuda, data, block) == want, ("mode 7", what)
        if below_cap:
            assert ctx.stats()["lazy_tiles"] == 0, ("mode 7", what, ctx.stats())
    finally:
        ctx.set_match_mode(0)
    assert _compress(ctx, cuda, data, block) == want, ("mode 0", what)
    if below_cap:   # every tile stayed in the sparse search: none handed on, none lazy
        rs, st = ctx.route_stats(), ctx.stats()
        assert rs["sparse"] > 0 and rs["handed_on"] == 0, (what, rs)
        assert st["lazy_tiles"] == 0, (what, st)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("length", LENGTHS)
def test_planted_copies(cuda, ctxs, L, block, length):
    ntiles = 3 + (length + block) % 4   # 3 .. 6 tiles
    ctx = ctxs(block, 6 * TILE)
    for d in DISTANCES:
        data = planted_input(1000 * length + d, ntiles, block, length, d)
        worst, cap = model_max_flagged(L, data, block)
        check_both_modes(ctx, cuda, data, block, 2 * worst <= cap, (block, length, d, worst))


def _three_copies(seed: int, extend_middle: bool) -> bytes:
    """the same 5-byte string three times inside one window of the second tile"""
    buf = bytearray(inputs.generate("rand", seed, 3 * TILE))
    a, b, c = TILE + 100, TILE + 900, TILE + 2000
    buf[b:b + 5] = buf[a:a + 5]
    buf[c:c + 5] = buf[a:a + 5]
    if extend_middle:   # the middle copy and the last agree on 9 bytes: the longest candidate wins
        buf[c:c + 9] = buf[b:b + 9]
    return bytes(buf)


@pytest.mark.parametrize("extend_middle", [True, False], ids=["longest_wins", "leftmost_wins"])
def test_three_copies(cuda, ctxs, extend_middle):
    data = _three_copies(61 + extend_middle, extend_middle)
    check_both_modes(ctxs(65536, 6 * TILE), cuda, data, 65536, True, extend_middle)


def _distinct_repeats(seed: int, count: int) -> bytes:
    """`count` distinct 3-byte repeats inside the second tile, 24 positions apart, 12 back each"""
    buf = bytearray(inputs.generate("rand", seed, 3 * TILE))
    for i in range(count):
        assert plant(buf, TILE + 50 + 24 * i, 12, 3)
    return bytes(buf)


def test_both_sides_of_the_cap(cuda, ctxs, L):
    out = (ctypes.c_uint32 * 4)()
    probe = np.zeros(8, dtype=np.uint8)
    assert L.fcx_debug_sparse_filter(ctypes.c_void_p(probe.ctypes.data), 4, None, out) == 0
    cap = out[1]
    assert 24 * 2 * cap + 50 <= TILE
    ctx = ctxs(65536, 6 * TILE)
    for count in (cap // 4, cap - 1, cap, cap + 1, 2 * cap):
        data = _distinct_repeats(90 + count, count)
        worst, _ = model_max_flagged(L, data, 65536)
        assert worst >= count
        check_both_modes(ctx, cuda, data, 65536, 2 * worst <= cap, (count, worst))


def test_routed_rand_and_text_blocks(cuda, L):
    """rand blocks alternating with text blocks, the planted repeats in the rand blocks: the
    classifier files the rand tiles for the sparse unit; those whose flagged keys exceed the cap
    are not sparse and go on to the no-filter list once the units run listed.  (No lazy-tile bar
    here: in some calls one tile of this input is left to the stitch, with the 17-bit filter as
    well and more often.  The cause is the extension budget of the bucket search: a query inside a
    planted run of period 1-3 and 257-300 bytes has hundreds of candidates of 12 bytes or more;
    oldest first one extension serves, in pass B as many extend as arrive before the oldest has
    written the best -- more than 24 in some calls.  Without those plants the input never showed
    a lazy tile, with them alone it did: DESIGN.md §3, test_gpu_match_edges.py.  The bytes are the
    oracle's either way.)"""
    block, nblocks = 65536, 32
    rng = random.Random(7)
    parts = []
    for i in range(nblocks):
        if i % 2:
            parts.append(inputs.generate("text", 300 + i, block))
            continue
        buf = bytearray(inputs.generate("rand", 300 + i, block))
        for t in range(TILE, block, TILE):   # one plant per tile, across its start now and then
            length, d = rng.choice(LENGTHS), rng.choice(DISTANCES)
            plant(buf, t + rng.choice((0, -1, 7, 1500, TILE - length)), d, length)
        parts.append(bytes(buf))
    data = b"".join(parts)
    want = oracle.compress_file(data, block)
    ctx = mc.Context(0, block, len(data))
    try:
        for call in range(3):
            assert _compress(ctx, cuda, data, block) == want, call
            rs = ctx.route_stats()
            assert rs["sparse"] > 0, rs
            if call > 0:   # listed: the tiles above the cap went on to the no-filter list
                assert rs["handed_on"] > 0 and rs["rest"] == 0, rs
    finally:
        ctx.close()
