// fcx_route_plan.h — the host's plan of a routed call's match launches: pure integer arithmetic on
// the estimates of each unit's share of the tiles (fcx_route.hip).  Host-only and free
// of HIP, so the thresholds are tested without a GPU (tests/test_route_plan.py through
// fcx_debug_route_plan).  The output bytes do not depend on any of it: a plan only costs time.
#pragma once
#include <algorithm>
#include <cstdint>

namespace fcx {

// Lists 0-3 are the match units (fcx_match.hip, one per row of the Makefile's unit table); list 4 the
// uniform unit (fcx_match_uniform.hip: tiles whose sample is one byte value, checked over their whole
// window, the others handed on to runs).  The search units in launch order: the sparse and runs units
// hand tiles on to the no-filter unit's list, so it comes last.
enum : uint32_t {
    kRouteSparse = 0, kRouteRuns = 1, kRouteKey4 = 2, kRouteNoFilter = 3, kSearchUnits = 4,
    kRouteUniform = 4, kRoutes = 5
};
// route counters of a call (k_classify, the units' hand-ons, the host's cover mark): [0, kRoutes)
// list lengths, then these
constexpr uint32_t kRcNfFiled = 5;    // tiles the classifier filed as no-filter (its list grows by hand-ons)
constexpr uint32_t kRcValid = 6;      // tiles with bytes
constexpr uint32_t kRcCover = 7;      // the no-filter list's length at its listed launch
constexpr uint32_t kRcRunsFiled = 8;  // tiles the classifier filed as runs (its list grows by the uniform unit's hand-ons)
constexpr uint32_t kRouteWords = 16;

constexpr uint32_t kRouteMinTiles = 8;      // a unit expected to get fewer tiles is not launched (k_match_rest)
constexpr uint32_t kRestDirect = ~0u;       // RoutePlan::grid: a direct launch (over every tile of the shard)

// each unit's expected tiles among the ntg of a shard, from a recent call's list lengths cnt out of its
// valid tiles with bytes (rounded up; any values are a valid estimate, they only size the grids)
inline void route_estimate(const uint64_t cnt[kRoutes], uint64_t valid, uint32_t ntg, uint64_t est[kRoutes]) {
    const uint64_t v = std::max<uint64_t>(valid, 1);
    for (uint32_t u = 0; u < kRoutes; u++) est[u] = (cnt[u] * ntg + v - 1) / v;
}

// What a context keeps of a recent routed call for the next calls' estimates.
struct RouteHint {
    bool have = false;            // a routed call has run: the estimates below are set
    uint64_t cnt[kRoutes] = {};   // tiles per list (after the hand-ons) of a recent call ...
    uint64_t valid = 0;           // ... out of its tiles with bytes
    uint64_t fix = 0;             // its hand-ons plus its lazy tiles (k_tree): > 0 keeps every unit listed
    // takes over a call's route counters and lazy tiles; counters without a tile with bytes (nothing has
    // landed in them yet) leave the estimate as it was
    void adopt(const uint32_t counters[kRouteWords], uint32_t lazy) {
        if (!counters[kRcValid]) return;
        for (uint32_t u = 0; u < kRoutes; u++) cnt[u] = counters[u];
        valid = counters[kRcValid];
        fix = (uint64_t)(uint32_t)(counters[kRouteNoFilter] - counters[kRcNfFiled]) + lazy;
    }
};

struct RoutePlan {
    uint32_t ugrid;                 // the uniform unit's grid (launched first)
    uint32_t best;                  // the search unit with the largest estimate (ties: the lowest index)
    bool direct;                    // best runs direct, over every tile of the shard ...
    bool every;                     // ... with the unrouted kernel's exact code
    uint32_t order[kSearchUnits];   // the search units in launch order
    uint32_t grid[kSearchUnits];    // per unit: its listed grid (0: not launched), kRestDirect for the direct unit
};

// est: the shard's expected tiles per list; ntg: its tiles; fix: a recent call had hand-ons or lazy
// tiles (k_tree) -- tiles its units' samples misfiled
inline RoutePlan plan_route(const uint64_t est[kRoutes], uint32_t ntg, bool fix) {
    RoutePlan p{};
    // the uniform unit is looped: any grid covers its list; a multiple of 8 for its XCD split.  At
    // least 2048 one-wave workgroups (≈ 3 µs when the list is empty), so an unforeseen list is still
    // taken by 8 waves per CU
    p.ugrid = (uint32_t)std::min<uint64_t>(8192, std::max<uint64_t>(2048, (est[kRouteUniform] + 7) / 8 * 8));
    // the unit expected to take most of the tiles (at least half) runs first, direct over every
    // tile of the shard: it drops the others by their kind byte -- or, when the estimate gives
    // it (nearly) all tiles, it searches every tile with the unrouted kernel's exact code, and
    // the few tiles of other kinds are searched again by their own units afterwards (the last
    // writer's outputs are complete).  The others run over their lists.
    for (uint32_t u = 1; u < kSearchUnits; u++)
        if (est[u] > est[p.best]) p.best = u;
    // (fix keeps every unit listed: only listed sparse / runs launches hand misfiled tiles on)
    p.direct = 2 * est[p.best] >= ntg && !fix;
    p.every = p.direct && 64 * est[p.best] >= 63ull * ntg;
    uint32_t no = 0;
    if (p.direct) p.order[no++] = p.best;
    for (uint32_t u = 0; u < kSearchUnits; u++) {
        if (p.direct && u == p.best) {
            p.grid[u] = kRestDirect;
            continue;
        }
        p.order[no++] = u;
        // a small margin over the estimate (its excess workgroups exit at once); the no-filter
        // list also takes the tiles the sparse / runs units hand on
        p.grid[u] = est[u] >= kRouteMinTiles ? (uint32_t)std::min<uint64_t>(est[u] + est[u] / 16 + 32, ntg) : 0u;
    }
    return p;
}

// The first entry of a unit's list that its remainder (k_match_rest_<unit>) owns, given the unit's
// RoutePlan::grid: start, or where word >= 0 the smaller of start and that route counter, which only
// the device knows when the remainder runs (RouteRest::start / start_dev).
struct RestStart {
    uint32_t start;
    int word;
    bool none() const { return start == ~0u && word < 0; }   // nothing left: no remainder launch
};
inline RestStart rest_start(uint32_t grid, uint32_t unit) {
    // a direct launch (first) has every entry of its list: no remainder -- but the no-filter list grows
    // by later hand-ons, past the entries the classifier filed
    if (grid == kRestDirect) return {~0u, unit == kRouteNoFilter ? (int)kRcNfFiled : -1};
    // a listed launch has the entries below its grid (0: not launched).  The no-filter launch covers
    // min(grid, its count at the cover mark); later hand-ons land past that count, possibly below the grid
    return {grid, unit == kRouteNoFilter && grid ? (int)kRcCover : -1};
}
// the same with the call's counters in hand, as the device takes it (fcx_ctx_route_stats)
inline uint32_t rest_start(uint32_t grid, uint32_t unit, const uint32_t counters[kRouteWords]) {
    const RestStart s = rest_start(grid, unit);
    if (s.none()) return counters[unit];
    return s.word >= 0 ? std::min(s.start, counters[s.word]) : s.start;
}

}  // namespace fcx
