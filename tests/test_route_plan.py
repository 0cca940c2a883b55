"""The routed call's launch plan (my_compress_amd/csrc/fcx_route_plan.h) through libfcx.so's development
exports: pure host arithmetic, no GPU.  The expected values are worked out by hand from the rules the
compress call has always applied: a unit's grid is est + est/16 + 32 capped at the
shard's tiles (0 below 8 expected tiles), the unit with the largest estimate (ties: the lowest list)
goes direct when 2 est >= tiles and no recent call misfiled tiles, with the unrouted code when
64 est >= 63 tiles, and it is launched first."""
import ctypes
import itertools

import pytest

import my_compress_amd as mc

SPARSE, RUNS, K4, NF, UNIFORM = range(5)
DIRECT = 0xFFFFFFFF      # a direct unit's grid in the plan
NF_FILED, VALID, COVER = 5, 6, 7   # route counter words past the five list lengths


@pytest.fixture(scope="module")
def L():
    lib = mc.lib()
    lib.fcx_debug_route_plan.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_uint32)]
    lib.fcx_debug_route_estimate.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.POINTER(ctypes.c_uint64)]
    lib.fcx_debug_rest_start.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.fcx_debug_rest_start.restype = ctypes.c_uint32
    lib.fcx_debug_route_hint.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                         ctypes.c_uint32]
    return lib


def plan(L, est, ntg=1024, fix=0):
    out = (ctypes.c_uint32 * 12)()
    assert L.fcx_debug_route_plan((ctypes.c_uint64 * 5)(*est), ntg, fix, out) == 0
    v = list(out)
    return {"ugrid": v[0], "best": v[1], "direct": bool(v[2]), "every": bool(v[3]), "order": v[4:8], "grid": v[8:12]}


def test_nothing_expected(L):
    p = plan(L, [0, 0, 0, 0, 0])
    assert (p["direct"], p["every"]) == (False, False)
    assert p["grid"] == [0, 0, 0, 0] and p["order"] == [0, 1, 2, 3] and p["ugrid"] == 2048


@pytest.mark.parametrize("u", [SPARSE, RUNS, K4, NF])
def test_minimum_tiles_and_margin(L, u):
    est = [0] * 5
    est[u] = 7
    assert plan(L, est)["grid"] == [0, 0, 0, 0]
    est[u] = 8
    want = [0] * 4
    want[u] = 40   # 8 + 8 // 16 + 32
    p = plan(L, est)
    assert p["grid"] == want and not p["direct"] and p["best"] == u


def test_grid_clamps_to_the_groups_tiles(L):
    p = plan(L, [19, 19, 0, 0, 0], ntg=40)   # 19 + 1 + 32 = 52 > 40; 2 * 19 < 40: nobody direct
    assert not p["direct"] and p["grid"] == [40, 40, 0, 0]


def test_three_way_split(L):
    p = plan(L, [341, 341, 0, 342, 0])
    assert not p["direct"] and p["best"] == NF
    assert p["order"] == [0, 1, 2, 3] and p["grid"] == [394, 394, 0, 395]


def test_direct_from_half_of_the_tiles(L):
    p = plan(L, [0, 0, 0, 512, 0])
    assert p["direct"] and not p["every"] and p["best"] == NF
    assert p["order"] == [NF, SPARSE, RUNS, K4] and p["grid"] == [0, 0, 0, DIRECT]
    p = plan(L, [0, 0, 0, 511, 0])
    assert not p["direct"] and p["order"] == [0, 1, 2, 3] and p["grid"] == [0, 0, 0, 574]   # 511 + 31 + 32


def test_tie_goes_to_the_lowest_list(L):
    p = plan(L, [512, 0, 0, 512, 0])
    assert p["best"] == SPARSE and p["direct"] and not p["every"]
    assert p["order"] == [0, 1, 2, 3] and p["grid"] == [DIRECT, 0, 0, 576]   # 512 + 32 + 32


def test_unrouted_code_from_63_in_64(L):
    p = plan(L, [0, 0, 0, 1007, 0])   # 64 * 1007 = 64448 < 63 * 1024 = 64512
    assert p["direct"] and not p["every"]
    p = plan(L, [0, 0, 0, 1008, 0])   # 64 * 1008 = 64512
    assert p["direct"] and p["every"] and p["grid"] == [0, 0, 0, DIRECT]


def test_direct_unit_is_launched_first(L):
    p = plan(L, [17, 0, 0, 1007, 0])
    assert p["direct"] and p["best"] == NF
    assert p["order"] == [NF, SPARSE, RUNS, K4] and p["grid"] == [50, 0, 0, DIRECT]   # 17 + 1 + 32


def test_misfiled_tiles_keep_every_unit_listed(L):
    p = plan(L, [0, 0, 0, 1024, 0], fix=1)
    assert not p["direct"] and not p["every"]
    assert p["order"] == [0, 1, 2, 3] and p["grid"] == [0, 0, 0, 1024]   # 1024 + 64 + 32 clamped
    assert plan(L, [0, 0, 0, 1024, 0], fix=0)["every"]


@pytest.mark.parametrize("est_uniform,ugrid", [(0, 2048), (2041, 2048), (2049, 2056), (100000, 8192)])
def test_uniform_grid(L, est_uniform, ugrid):
    assert plan(L, [0, 0, 0, 0, est_uniform])["ugrid"] == ugrid


@pytest.mark.parametrize("ntg", [0, 1, 7, 8, 1024])
def test_any_estimates_give_a_launchable_plan(L, ntg):
    """every unit once in the order, listed grids within the group's tiles, one direct unit at most and
    that one first (the estimates are unchecked values from a recent call)"""
    for est in itertools.product([0, 1, 7, 8, 600, 1 << 33], repeat=4):
        for fix in (0, 1):
            p = plan(L, list(est) + [3], ntg, fix)
            assert sorted(p["order"]) == [0, 1, 2, 3]
            direct = [u for u in range(4) if p["grid"][u] == DIRECT]
            assert direct == ([p["best"]] if p["direct"] else []) and not (fix and direct)
            assert all(p["grid"][u] <= ntg for u in range(4) if u not in direct)
            assert not direct or p["order"][0] == direct[0]
            assert p["every"] <= p["direct"] and p["ugrid"] == 2048


def estimate(L, cnt, valid, ntg):
    est = (ctypes.c_uint64 * 5)()
    assert L.fcx_debug_route_estimate((ctypes.c_uint64 * 5)(*cnt), valid, ntg, est) == 0
    return list(est)


def test_estimate_rounds_up_and_survives_no_valid_tiles(L):
    assert estimate(L, [3, 0, 1000, 10, 999], 1000, 100) == [1, 0, 100, 1, 100]
    assert estimate(L, [3, 0, 0, 0, 1], 0, 100) == [300, 0, 0, 0, 100]   # valid 0 counts as 1


def rest_start(L, grid, unit, lists, nf_filed=0, cover=0):
    c = (ctypes.c_uint32 * 16)(*lists)
    c[NF_FILED], c[COVER] = nf_filed, cover
    return L.fcx_debug_rest_start(grid, unit, c)


def test_rest_starts(L):
    lists = [100, 200, 300, 400, 0]
    # a listed launch: its remainder starts past the grid (0: not launched, the whole list)
    for u in (SPARSE, RUNS, K4):
        assert rest_start(L, 40, u, lists, cover=7) == 40
        assert rest_start(L, 0, u, lists, cover=7) == 0
    assert rest_start(L, 0, NF, lists, nf_filed=350, cover=7) == 0
    # direct sparse / runs / 4-byte: the launch had every entry, nothing is left
    for u in (SPARSE, RUNS, K4):
        assert rest_start(L, DIRECT, u, lists, nf_filed=350, cover=7) == lists[u]
    # direct no-filter: the hand-ons past the entries the classifier filed are left
    assert rest_start(L, DIRECT, NF, lists, nf_filed=350, cover=7) == 350
    # listed no-filter: its launch covered the smaller of its grid and the list's length at the cover
    # mark; hand-ons that arrive later sit past that length, also where it is below the grid
    assert rest_start(L, 395, NF, lists, nf_filed=290, cover=300) == 300
    assert rest_start(L, 395, NF, lists, nf_filed=290, cover=398) == 395


def adopt(L, hint, lists, valid, nf_filed, lazy):
    """the estimate (cnt[5], valid, fix) after RouteHint::adopt of a call's counters and lazy tiles"""
    c = (ctypes.c_uint32 * 16)(*lists)
    c[NF_FILED], c[VALID], c[COVER] = nf_filed, valid, 12345   # (the cover mark plays no part)
    h = (ctypes.c_uint64 * 7)(*hint)
    assert L.fcx_debug_route_hint(h, c, lazy) == 0
    return list(h)


def test_hint_ignores_counters_without_valid_tiles(L):
    prev = [10, 20, 30, 40, 50, 150, 3]
    assert adopt(L, prev, [1, 2, 3, 9, 5], valid=0, nf_filed=4, lazy=7) == prev
    assert adopt(L, [0] * 7, [1, 2, 3, 9, 5], valid=0, nf_filed=4, lazy=7) == [0] * 7


def test_hint_fix_is_hand_ons_plus_lazy_tiles(L):
    prev = [10, 20, 30, 40, 50, 150, 3]
    lists = [100, 200, 300, 400, 24]
    # the no-filter list holds 400 tiles, 390 of them filed by the classifier: 10 hand-ons, + 2 lazy tiles
    assert adopt(L, prev, lists, valid=1024, nf_filed=390, lazy=2) == lists + [1024, 12]
    assert adopt(L, prev, lists, valid=1024, nf_filed=400, lazy=2) == lists + [1024, 2]
    assert adopt(L, prev, lists, valid=1024, nf_filed=399, lazy=0) == lists + [1024, 1]
    clean = adopt(L, prev, lists, valid=1024, nf_filed=400, lazy=0)   # (a clean call clears an earlier fix)
    assert clean == lists + [1024, 0]
    # a nonzero fix keeps every unit listed, where the same estimates would send no-filter direct
    nf_most = [0, 0, 0, 1024, 0]
    for nf_filed, lazy in ((1023, 0), (1024, 1)):
        h = adopt(L, [0] * 7, nf_most, valid=1024, nf_filed=nf_filed, lazy=lazy)
        assert h[6] == 1
        p = plan(L, estimate(L, h[:5], h[5], 1024), 1024, fix=int(h[6] != 0))
        assert not p["direct"] and p["order"] == [0, 1, 2, 3] and p["grid"] == [0, 0, 0, 1024]
    h = adopt(L, [0] * 7, nf_most, valid=1024, nf_filed=1024, lazy=0)
    assert plan(L, estimate(L, h[:5], h[5], 1024), 1024, fix=int(h[6] != 0))["grid"] == [0, 0, 0, DIRECT]


def test_cold_adoption_is_adopt_of_the_calls_own_counts(L):
    """a context's first routed call takes its own counts right after the classifier: every no-filter
    tile is a filed one and no tile is lazy yet, so the estimate is those counts with fix 0 -- what
    adopt makes of the same counters, whatever it held before"""
    lists = [7, 100, 0, 893, 24]
    want = lists + [1000, 0]
    assert adopt(L, [0] * 7, lists, valid=1000, nf_filed=893, lazy=0) == want
    assert adopt(L, [9, 9, 9, 9, 9, 45, 5], lists, valid=1000, nf_filed=893, lazy=0) == want
