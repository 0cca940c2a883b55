"""Every match unit at the places where the search decides something, against the oracle: the
crafted inputs of tests/match_craft.py (pinned on the CPU by tests/test_match_craft.py) through
the forced modes 1-7 (the general kernel's bucket search and whole-tile run table, then the
general, 4-byte-key, no-filter, runs and sparse units) and three routed calls (mode 0).  Bar: the
bytes equal oracle.compress_file's with the exhaustive finder, at block 65536 and at block 12293
(ragged last tiles, candidates cut off by a block start).  The lazy-tile and route counters are
evidence about the path taken, asserted only where the code leaves no choice; every test prints
them (`COUNTERS` lines) for DESIGN.md §3's table.
"""
import pytest

import match_craft as craft
import my_compress_amd as mc
import oracle

pytestmark = pytest.mark.gpu

TILE = craft.TILE
MODES = (1, 2, 3, 4, 5, 6, 7)
BLOCKS = (65536, 12293)
CAP = 8 * TILE
# the planted-copy matrix of test_gpu_sparse_filter.py (there through modes 7 and 0)
LENGTHS = (3, 4, 11, 12, 13, 257, 258, 259, 300)
DISTANCES = (1, 2, 3, 2046, 2047, 2048, 2049)
PLANT_BLOCKS = (65536, 12293, 5000)
UNITS = ("sparse", "runs", "key4", "nofilter", "uniform")


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(block: int, cap_bytes: int = CAP):
        key = (block, cap_bytes)
        if key not in made:
            made[key] = mc.Context(0, block, cap_bytes)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def run_modes(ctx, cuda, data: bytes, block: int, what, modes=MODES, routed: int = 3) -> dict:
    """`data` through the forced modes and then `routed` calls of mode 0 on the same context, every
    output compared with the oracle's; returns {mode: stats} and {0: [(stats, route_stats), ...]}"""
    import torch

    want = oracle.compress_file(data, block)
    head = mc.write_header(len(data), (len(data) + block - 1) // block)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)
    cap = mc.shard_bound(len(data), block)
    d_out = torch.empty(cap, dtype=torch.uint8, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def once():
        n = ctx.compress_shard(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, stream)
        return head + d_out[:n].cpu().numpy().tobytes()

    seen = {}
    try:
        for mode in modes:
            ctx.set_match_mode(mode)
            got = once()
            seen[mode] = ctx.stats()
            assert got == want, ("mode", mode, what, seen[mode])
    finally:
        ctx.set_match_mode(0)
    seen[0] = []
    for call in range(routed):
        got = once()
        seen[0].append((ctx.stats(), ctx.route_stats()))
        assert got == want, ("mode 0, call", call, what, seen[0][-1])
    return seen


def lazy_of(seen, mode):
    """(lazy tiles, lazy evaluations) of a mode.  lazy_tiles: tiles the match kernel left positions
    unknown in; lazy_evals: positions the stitch evaluated itself (also a few per block on its
    walks between speculative chains, so it is above zero without any lazy tile).  Mode 0: the
    largest of its estimated calls -- a context's cold first call launches the sparse unit direct
    over every tile, without the hand-on to the no-filter list (test_gpu_route.py), so a tile the
    sparse filter refuses is lazy there by construction"""
    sts = [s for s, rs in seen[0] if not rs["cold"]] if mode == 0 else [seen[mode]]
    return max(s["lazy_tiles"] for s in sts), max(s["lazy_evals"] for s in sts)


def report(family, case, rows):
    """rows: {(mode, label): [(lazy tiles, lazy evals), ...]} -> one COUNTERS line each"""
    for (mode, label), v in sorted(rows.items()):
        print(f"COUNTERS {family} {case} mode={mode} {label} inputs={len(v)} "
              f"lazy_tiles_max={max(t for t, _ in v)} lazy_inputs={sum(t > 0 for t, _ in v)} "
              f"lazy_evals_max={max(e for _, e in v)}")


# ---- a. planted copies through every unit ----
@pytest.mark.parametrize("block", PLANT_BLOCKS)
@pytest.mark.parametrize("length", LENGTHS)
def test_planted_copies_every_unit(cuda, ctxs, block, length):
    ntiles = 3 + (length + block) % 4   # 3 .. 6 tiles
    ctx = ctxs(block)
    for d in DISTANCES:
        data = craft.planted_input(1000 * length + d, ntiles, block, length, d)
        run_modes(ctx, cuda, data, block, (block, length, d), modes=(1, 2, 3, 4, 5, 6), routed=0)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("length", craft.SLAB_LENGTHS)
def test_slab_edge_plants(cuda, ctxs, block, length):
    """queries on both sides of an insertion slab's edge, their candidates 2046 / 2047 / 2048 back:
    the bucket counters read during passes s - 5 and s + 1 must keep the first and drop the last"""
    ctx = ctxs(block)
    for d in craft.SLAB_DISTANCES:
        for delta in craft.SLAB_DELTAS:
            data = craft.slab_edge_input(7000 + 10 * length + d, block, length, d, delta)
            run_modes(ctx, cuda, data, block, (block, length, d, delta))


# ---- b. extension budget and skip rule ----
NO_LAZY_MODES = (1, 3, 4, 5, 0)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("filler", ["rand", "text"])
@pytest.mark.parametrize("K", craft.STAIR_KS)
def test_extension_budget(cuda, ctxs, block, filler, K):
    """K candidates of 12 bytes or more for the query at q.  Up to K = 24 no arrival order can spend
    more than the 24 extensions of a query's budget, so the bucket search may leave no tile to the
    stitch: asserted on rand filler (nothing else in the tile is long or frequent) for modes 1, 3,
    4, 5 and the estimated calls of mode 0, which run right after a call with lazy tiles and so
    keep the units listed: the sparse unit hands the tile on to the no-filter list.

    Mode 7 is not among them.  The supposition was that only the budget could make the sparse unit
    leave a tile lazy; it never searches these tiles.  The copies repeat hundreds of keys, the
    unit's filter keeps a tile up to 64 flagged keys (test_match_craft.py checks the count), and a
    tile it refuses takes the whole-tile run table when the unit is forced, which a rand tile's
    runs overflow: every position unknown, for every K.  So mode 7 must leave lazy tiles here (the
    runs unit, mode 6, refuses the tile in the same way); that is asserted instead.

    K = 25 and 36 are recorded, not asserted.  Pass A counts a query's extensions in its packed
    word, pass B counts from zero in the hot slot (h_x), so a query has 24 in each: `up`, which
    extends every copy in any order, is lost at K = 25 only if all 25 fall in one pass.  In pass B
    64 candidates read the slot's best before any of them has written it, so `down` and `flat`
    extend as many copies as share a chunk of 64 with the oldest."""
    ctx = ctxs(block)
    rows = {}
    for order in craft.ORDERS:
        for q in craft.STAIR_QS:
            data = craft.staircase(craft.stair_seed(K), K, order, q, filler)
            if block < len(data):   # the block start 1000 before q: the older copies are cut off
                data = craft.cut_by_block(data, block, q - 1000, 900 + K, filler)
            seen = run_modes(ctx, cuda, data, block, (block, filler, K, order, q))
            for mode in MODES + (0,):
                rows.setdefault((mode, order), []).append(lazy_of(seen, mode))
    report("staircase", f"block={block} filler={filler} K={K}", rows)
    if K <= craft.EXT_BUDGET and filler == "rand" and block == 65536:
        for mode in NO_LAZY_MODES:
            for order in craft.ORDERS:
                assert max(t for t, _ in rows[(mode, order)]) == 0, (mode, order, K, rows[(mode, order)])
    if filler == "rand" and block == 65536:
        for order in craft.ORDERS:
            assert min(t for t, _ in rows[(7, order)]) > 0, (order, K, rows[(7, order)])


# ---- c. hot keys ----
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("marker", [craft.MARKER4, craft.MARKER3], ids=["key4", "key3"])
def test_hot_keys(cuda, ctxs, block, marker):
    """one key ~68 times in every window: the marker queries' bucket ranges are the long ones of
    their waves (pass B), and their match is the leftmost of equal candidates, or the longer of an
    old and a recent one.  The 3-byte marker in mode 4 is the 4-byte-key unit's fallback (kNeed3:
    no candidate shares four bytes)."""
    ctx = ctxs(block)
    cases = [("plain", {})] + [(v, {"variant": v}) for v in craft.HOT_VARIANTS]
    cases += [(f"stairs{K}{order}", {"stairs": (K, order)}) for K in (25, 36) for order in craft.ORDERS]
    rows = {}
    for name, kw in cases:
        data = craft.hot_key(5, marker, **kw)
        if block < len(data):
            data = craft.cut_by_block(data, block, craft.HOT_Q - 1000, 77)
        seen = run_modes(ctx, cuda, data, block, (block, marker, name))
        for mode in MODES + (0,):
            rows.setdefault((mode, "stairs" if "stairs" in kw else "planted"), []).append(lazy_of(seen, mode))
    report("hot_key", f"block={block} marker={marker.decode()}", rows)
    if marker == craft.MARKER4 and block == 65536:
        # 68 candidates of 4 bytes and at most two of 18: nowhere near 24 extensions or 1024 entries
        for mode in (1, 3, 4, 5):
            assert max(t for t, _ in rows[(mode, "planted")]) == 0, (mode, rows[(mode, "planted")])


# ---- d. run tables ----
@pytest.mark.parametrize("block", BLOCKS)
def test_run_ramp(cuda, block):
    """runs growing from 1 to 14 bytes: window runs on both sides of kRunBudget (512) at
    neighbouring positions, image runs on both sides of kRunTile (1024), stitch windows on both
    sides of kStRunCap (1020).  In the run-table modes (2: whole tiles of the general kernel, 6:
    the runs unit) a window of more than 512 runs is kUnknown in run_match_wave and must be
    evaluated by the stitch (nlazy++ in k_stitch): lazy_evals > 0, in a tile counted lazy.  Routed, the ramp's tiles are
    filed to more than one unit.  (A context of its own: its first routed call is the cold one.)"""
    data = craft.run_ramp(2)
    ctx = mc.Context(0, block, len(data))
    try:
        seen = run_modes(ctx, cuda, data, block, (block, "ramp"))
    finally:
        ctx.close()
    rows = {(mode, "ramp"): [lazy_of(seen, mode)] for mode in MODES + (0,)}
    report("run_ramp", f"block={block}", rows)
    for call, (_st, rs) in enumerate(seen[0]):
        print(f"COUNTERS run_ramp block={block} call={call} route={rs}")
        assert rs["cold"] == (call == 0), rs
        assert sum(rs[u] > 0 for u in UNITS) > 1, (call, rs)
    for mode in (2, 6):
        assert seen[mode]["lazy_evals"] > 0 and seen[mode]["lazy_tiles"] > 0, (mode, seen[mode])


PERIODS = craft.run_periods()


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", sorted(PERIODS))
def test_run_periods(cuda, ctxs, block, name):
    """periodic run patterns: ext over equal (byte, length) runs up to the cap, ext ending on a
    length mismatch, windows of exactly kRunBudget runs (a4b4) and above it (a4b3), the block end
    met with a shrinking cap, and (`z_`) windows whose first run is clipped.  a8b8 stays inside
    every budget (256 runs per window, 801 per image), so the run-table modes leave nothing lazy."""
    data = PERIODS[name]
    seen = run_modes(ctxs(block), cuda, data, block, (block, name))
    rows = {(mode, name): [lazy_of(seen, mode)] for mode in MODES + (0,)}
    report("run_periods", f"block={block}", rows)
    if name.endswith("a8b8"):
        for mode in (2, 6, 0):
            assert lazy_of(seen, mode)[0] == 0, (mode, name, seen[mode])
