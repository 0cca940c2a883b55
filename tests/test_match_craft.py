"""tests/match_craft.py pinned on the CPU: every crafted input reaches the place of the match
search it is built for (checked with the oracle's parse and with plain counts over the bytes), so
that a later edit of a builder cannot silently stop reaching an edge.  The GPU side is
tests/test_gpu_match_edges.py."""
import numpy as np
import pytest

import inputs
import match_craft as craft

BLOCK = 65536


# ---- extension budget / skip rule ----
@pytest.mark.parametrize("filler", ["rand", "text"])
@pytest.mark.parametrize("K", craft.STAIR_KS)
def test_staircase_token_at_q(filler, K):
    for order in craft.ORDERS:
        for q in craft.STAIR_QS:
            data = craft.staircase(craft.stair_seed(K), K, order, q, filler)
            assert len(data) == 3 * craft.TILE
            tm = craft.token_map(data, BLOCK)
            assert tm.get(q) == craft.stair_token(order, K), (filler, K, order, q, tm.get(q))


@pytest.mark.parametrize("K", craft.STAIR_KS)
def test_staircase_extensions_by_arrival_order(K):
    """what the orders are for: oldest first (pass A of the bucket scan), `up` spends one extension
    per copy -- K, past the budget of 24 from K = 25 -- while `down` and `flat` spend one, every later
    copy being skipped.  Newest first (one of pass B's possible orders) every order spends K: the
    rule skips only candidates right of the best.  Whatever the order, at most K are spent: K <= 24
    can never exhaust the budget."""
    q = craft.STAIR_QS[0]
    for order, oldest_first, newest_first in (("up", K, K), ("down", 1, K), ("flat", 1, K)):
        data = craft.staircase(craft.stair_seed(K), K, order, q, "rand")
        copies = craft.stair_copies(q, K)
        assert craft.extensions_in_order(data, q, copies) == oldest_first, order
        assert craft.extensions_in_order(data, q, copies[::-1]) == newest_first, order
    assert (K > craft.EXT_BUDGET) == (K in (25, 36))


@pytest.mark.parametrize("K", craft.STAIR_KS)
def test_staircase_tile_is_not_sparse(K):
    """the copies repeat far more keys than the sparse unit's filter accepts in a window (64): that
    unit does not search a staircase tile itself, whatever K is (a rand tile without a staircase
    repeats a handful)"""
    for order in craft.ORDERS:
        for q in craft.STAIR_QS:
            data = craft.staircase(craft.stair_seed(K), K, order, q, "rand")
            assert craft.window_repeats(data, q) > 3 * craft.SF_FLAG_CAP, (K, order, q)
    assert craft.window_repeats(inputs.generate("rand", 3, 3 * craft.TILE), craft.TILE) < craft.SF_FLAG_CAP // 4


# ---- hot keys ----
@pytest.mark.parametrize("marker", [craft.MARKER4, craft.MARKER3])
def test_hot_key_variants(marker):
    for variant in craft.HOT_VARIANTS:
        data = craft.hot_key(5, marker, variant=variant)
        assert craft.token_map(data, BLOCK).get(craft.HOT_Q) == craft.hot_winner(variant, marker), variant
    for K in (25, 36):
        for order in craft.ORDERS:
            data = craft.hot_key(5, marker, stairs=(K, order))
            assert craft.token_map(data, BLOCK).get(craft.HOT_Q) == craft.stair_token(order, K), (K, order)
            # the staircase's long candidates share the bucket range with the markers' short ones
            window = data[craft.HOT_Q - craft.WIN:craft.HOT_Q]
            assert window.count(marker) >= 60, window.count(marker)


def test_hot_key_sites():
    data = craft.hot_key(5, craft.MARKER4)
    tm = craft.token_map(data, BLOCK)
    sites = craft.marker_sites(data, craft.MARKER4)
    assert len(sites) == 409
    # the leftmost of 68 equal candidates, at the window's far edge
    assert sum(tm.get(p) == (2040, 4) for p in sites) >= 150
    data = craft.hot_key(5, craft.MARKER3)
    tm = craft.token_map(data, BLOCK)
    sites = craft.marker_sites(data, craft.MARKER3)
    # no candidate agrees on a fourth byte: the 4-byte-key unit finds none and falls back (kNeed3)
    assert sum(p in tm and tm[p][1] == 3 for p in sites) >= 100


# ---- run tables ----
RAMP_SEED = 2


def test_run_ramp_crosses_every_budget():
    data = craft.run_ramp(RAMP_SEED)
    assert len(data) == 8 * craft.TILE
    w = craft.window_runs(data, BLOCK)
    assert (w > craft.RUN_BUDGET).sum() >= 1000 and (w <= craft.RUN_BUDGET).sum() >= 1000
    assert (w == craft.RUN_BUDGET).any() and (w == craft.RUN_BUDGET + 1).any()
    # neighbouring positions on different sides of the budget
    assert ((w[1:] > craft.RUN_BUDGET) != (w[:-1] > craft.RUN_BUDGET)).sum() >= 2
    im = craft.image_runs(data, BLOCK)
    assert min(im) <= craft.RUN_TILE < max(im), im
    assert any(abs(r - craft.RUN_TILE) <= 10 for r in im), im
    st = craft.stitch_runs(data, BLOCK)
    assert (st > craft.ST_RUN_CAP).any() and (st <= craft.ST_RUN_CAP).any()
    # positions the match kernel's run table gives up on whose stitch window fits its table, and
    # positions where both give up (lazy_match)
    assert ((w > craft.RUN_BUDGET) & (st < craft.ST_RUN_CAP)).any()
    assert ((w > craft.RUN_BUDGET) & (st > craft.ST_RUN_CAP)).any()


def test_run_ramp_bytes():
    data = craft.run_ramp(RAMP_SEED)
    assert set(data) == set(b"abc")
    a = np.frombuffer(data, dtype=np.uint8)
    starts = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    lens = np.diff(np.r_[starts, len(a)])
    n = len(lens)
    # the mean run length grows along the buffer: 1 .. 14 asked for
    assert lens[:n // 8].mean() < 2.5 and lens[-n // 8:].mean() > 8


def test_run_periods():
    P = craft.run_periods()
    assert set(P) == {z + name for name in craft.RUN_PATTERNS for z in ("", "z_")}
    for name, data in P.items():
        assert len(data) == craft.RUN_PERIOD_N + (craft.RUN_PERIOD_LEAD if name.startswith("z_") else 0)
    w = craft.window_runs(P["a4b4"], BLOCK)
    assert w.max() == craft.RUN_BUDGET                       # reaches the budget, never exceeds it
    w = craft.window_runs(P["a4b3"], BLOCK)
    assert w.max() == 585 and (w > craft.RUN_BUDGET).sum() > len(w) // 2
    for name in ("a8b8", "z_a8b8"):                          # inside every budget
        assert craft.window_runs(P[name], BLOCK).max() == 256
        assert max(craft.image_runs(P[name], BLOCK)) <= 801 < craft.RUN_TILE
        assert craft.stitch_runs(P[name], BLOCK).max() < craft.ST_RUN_CAP
    # behind the lead the early windows begin inside the 1500-byte run: a clipped first run
    lead = craft.RUN_PERIOD_LEAD
    assert P["z_a4b4"][:lead] == b"z" * lead and P["z_a4b4"][lead:] == P["a4b4"]
    # the near-repeat's halves agree for three runs and then differ in a run's length
    tm = craft.token_map(P["a3b5c2a3b4d"], BLOCK)
    assert tm.get(10) == (10, 7), tm.get(10)


# ---- slab-edge plants ----
@pytest.mark.parametrize("length", craft.SLAB_LENGTHS)
def test_slab_edge_plants(length):
    """the copy at 512 k + delta is the oracle's token there, at the planted distance while that
    is inside the window (2048 is not)"""
    for d in craft.SLAB_DISTANCES:
        for delta in craft.SLAB_DELTAS:
            data = craft.slab_edge_input(7000 + 10 * length + d, BLOCK, length, d, delta)
            tm = craft.token_map(data, BLOCK)
            sites = [2 * craft.TILE + craft.SLAB * k + delta for k in range(1, 8)]
            hit = sum(tm.get(p, (0, 0))[0] == d and tm[p][1] >= min(length, craft.MAXL - 1) for p in sites)
            if d <= craft.WIN:
                assert hit >= 6, (length, d, delta, [tm.get(p) for p in sites])
            else:
                assert hit == 0, (length, d, delta)
