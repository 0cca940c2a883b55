"""The sparse unit's two phases (fcx_match.hip under FCX_SPARSE, fcx_sparse_tail.hip)
against the oracle: k_match_sparse ends a tile after its equal-key search -- all literals when no two
R entries pair up, else R left in the tile's mtok slot for k_sparse_tail's one wave, else (more than
64 R entries, or an entry with more candidates than the extension budget) the queries stay in the
workgroup.  Seeded random bytes with planted copies at the places where that split can go wrong, each
input with the sparse unit forced (mode 7) and routed (mode 0, twice: the second call runs from the
first one's counts), at block sizes 1 MiB, 4097 and 5000.  Bar: the bytes equal the oracle's.
"""
import ctypes

import numpy as np
import pytest

import inputs
import my_compress_amd as mc
import oracle
from match_craft import geometry, plant

pytestmark = pytest.mark.gpu

TILE, HALO, WIN = 4096, 2048, 2047
N = 256 << 10
BLOCKS = (1 << 20, 4097, 5000)


def _sites(n: int, block: int):
    """(block start, block end, tile start) of a first tile and of a later tile, mid-buffer: where
    every case plants"""
    blocks, tiles = geometry(n, block)
    bs, be = blocks[len(blocks) // 2]
    ts = tiles[len(tiles) // 2]
    tb = next(b for b in blocks if b[0] <= ts < b[1])
    return [(bs, be, bs), (tb[0], tb[1], ts)]


def short_copies(buf, bs, be, t):      # 1. a 3-byte and a 4-byte copy wholly inside a tile
    plant(buf, t + 300, 100, 3)
    plant(buf, t + 700, 150, 4)


def halo_2047(buf, bs, be, t):         # 2. the source at distance exactly 2047 (in the left halo): a match
    plant(buf, max(t, bs + WIN) + 5, 2047, 6)


def halo_2048(buf, bs, be, t):         # 3. ... at exactly 2048: no match
    plant(buf, max(t, bs + 2048) + 40, 2048, 6)


def across_tile_end(buf, bs, be, t):   # 4. starts in a tile's last 3 positions, runs into the next
    end = t if t > bs else t + TILE   # a tile end inside the block, and the next two where the block has them
    for k, back in enumerate((2, 1, 3)):
        plant(buf, end + TILE * k - back, 500 + back, 20)


def three_equal_keys(buf, bs, be, t):  # 5. one key three times in a window: two flagged entries of one value
    a, b, c = t + 100, t + 900, t + 2000
    buf[b:b + 3] = buf[a:a + 3]
    buf[c:c + 3] = buf[a:a + 3]


def equal_candidates(buf, bs, be, t):  # 6. two candidates of equal length: the leftmost wins
    a, b, c = t + 120, t + 1000, t + 1900
    buf[b:b + 5] = buf[a:a + 5]
    buf[c:c + 5] = buf[a:a + 5]
    buf[c + 5] = (buf[a + 5] + 1) & 0xFF
    buf[b + 5] = (buf[a + 5] + 2) & 0xFF


def long_copies(buf, bs, be, t):       # 7. 12, 13 and 258+ bytes: the extension path and the cap
    plant(buf, t + 800, 700, 12)
    plant(buf, t + 900, 650, 13)
    plant(buf, t + 1300, 1000, 258)
    plant(buf, t + 2400, 900, 300)


def block_edges(buf, bs, be, t):       # 8. a match within 4 bytes of the block's end, one at block position 1
    plant(buf, be - 7, 100, 7)
    plant(buf, bs + 1, 1, 5)


def many_r_entries(buf, bs, be, t):    # 9. more than 64 R entries within the flag cap: 18 keys four times each
    for i in range(18):
        a = t + 40 + 11 * i
        for r in (1, 2, 3):
            buf[a + 260 * r:a + 260 * r + 3] = buf[a:a + 3]
    plant(buf, t + 1500, 1, 100)       # ... and a run of one key (past the flag cap: not sparse)


def budget_runs(buf, bs, be, t):       # 10. queries with more than 24 long candidates: period 1 and 2
    plant(buf, t + 1500, 1, 40)
    plant(buf, t + 2500, 2, 56)


CASES = (short_copies, halo_2047, halo_2048, across_tile_end, three_equal_keys, equal_candidates, long_copies,
         block_edges, many_r_entries, budget_runs)


def _case_input(case, block: int) -> bytes:
    buf = bytearray(inputs.generate("rand", 500 + CASES.index(case), N))
    for bs, be, t in _sites(N, block):
        case(buf, bs, be, t)
    return bytes(buf)


def _many_plants(block: int) -> bytes:
    """a copy in every tile of 1 MiB: every tile goes through the tail kernel"""
    n = 1 << 20
    buf = bytearray(inputs.generate("rand", 77, n))
    r = inputs._lcg(78)
    for t in range(0, n, TILE):
        length = (3, 4, 11, 12, 13, 40, 257, 258, 300)[(next(r) >> 8) % 9]
        plant(buf, t + (next(r) >> 8) % (TILE - 300), 1 + (next(r) >> 8) % 2200, length)
    return bytes(buf)


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


def _tail_count(ctx) -> int:
    f = mc.lib().fcx_debug_sparse_tail_count
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    out = ctypes.c_uint64(0)
    assert f(ctx._h, ctypes.byref(out)) == 0
    return out.value


def check_forced_and_routed(ctx, cuda, data: bytes, block: int, what):
    want = oracle.compress_file(data, block)
    ctx.set_match_mode(7)   # the sparse unit forced
    try:
        assert _compress(ctx, cuda, data, block) == want, ("mode 7", what)
        forced = _tail_count(ctx)
    finally:
        ctx.set_match_mode(0)
    for call in range(2):
        assert _compress(ctx, cuda, data, block) == want, ("mode 0", call, what)
    return forced


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("case", CASES, ids=[c.__name__ for c in CASES])
def test_planted_case(cuda, ctxs, case, block):
    data = _case_input(case, block)
    listed = check_forced_and_routed(ctxs(block, 1 << 20), cuda, data, block, (case.__name__, block))
    assert listed > 0, (case.__name__, block)   # (the random tiles around the plants: about 4 in 10 are listed)


@pytest.mark.parametrize("block", BLOCKS)
def test_a_copy_in_every_tile(cuda, ctxs, block):
    data = _many_plants(block)
    check_forced_and_routed(ctxs(block, 1 << 20), cuda, data, block, ("every tile", block))


def pair_tiles(data: bytes, block: int):
    """tiles with a position whose 3-byte key occurs again at most 2047 back in its block (the
    position not the block's first, four bytes or more left in the block), and all tiles: the tiles
    phase 1 must list -- of equal keys in a window at most one is not flagged
    (tests/test_sparse_filter_model.py), so both are in R"""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint32)
    n = len(a)
    keys = a[:-2] | (a[1:-1] << 8) | (a[2:] << 16)
    order = np.argsort(keys, kind="stable")
    ks, ps = keys[order], order
    same = ks[1:] == ks[:-1]
    x, xp = ps[1:][same], ps[:-1][same]
    bs = x - x % block
    i = x - bs
    ok = (x - xp <= WIN) & (xp >= bs) & (i != 0) & (np.minimum(block, n - bs) - i >= 4)
    tiles = set(zip(bs[ok].tolist(), (i[ok] // TILE).tolist()))
    return len(tiles), sum((min(block, n - b) + TILE - 1) // TILE for b in range(0, n, block))


def test_listed_share_of_random_tiles(cuda, ctxs):
    """plain random bytes (seed 4, 1 MiB, one block): the tiles with an equal-key pair are listed, the
    others end in phase 1.  4096 positions x 2047 candidates / 2^24 keys = 0.5 pairs per tile, so
    1 - exp(-0.5) = 39 % of tiles on average; counted for this input: 118 of 256 (46 %).  A listed
    tile without such a pair needs two R entries -- a window has about 4 -- that agree in 19 key bits
    but not in 24: not one tile in 10 000."""
    block, n = 1 << 20, 1 << 20
    data = inputs.generate("rand", 4, n)
    pairs, tiles = pair_tiles(data, block)
    assert (pairs, tiles) == (118, 256)
    ctx = ctxs(block, 1 << 20)
    want = oracle.compress_file(data, block)
    ctx.set_match_mode(7)
    try:
        assert _compress(ctx, cuda, data, block) == want
        forced = _tail_count(ctx)
    finally:
        ctx.set_match_mode(0)
    assert _compress(ctx, cuda, data, block) == want
    routed = _tail_count(ctx)
    for listed in (forced, routed):
        print(f"listed {listed} of {tiles} tiles, {pairs} with an equal-key pair")
        assert 0.25 * tiles <= listed <= 0.55 * tiles, (listed, tiles)
    assert pairs <= forced <= pairs + 2, (forced, pairs)   # (routed, a tile may be filed for another unit)
