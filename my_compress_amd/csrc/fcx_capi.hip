// fcx_capi.hip — C ABI of the compress path: context, scratch layout in HBM and
// the launch sequence.  See include/fcx.h for the contract and the reference
// interfaces each entry point replaces.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_device.h"
#include "fcx_host.h"
#include "fcx_sparse_filter.h"
#include "fcx_sparse_tail.h"

using namespace fcx;

namespace {
thread_local std::string g_err;

inline uint32_t round16(uint64_t x) { return (uint32_t)((x + 15) & ~15ull); }

const char *kStageNames[] = {"route",        "match",       "stitch", "emit",   "hist",   "tree",
                             "block_layout", "scan_blocks", "zero",   "encode", "headers"};
constexpr int kNumStages = 11;

Layout make_layout(uint64_t n, uint32_t B) {
    Layout L;
    memset(&L, 0, sizeof(L));
    L.n = n;
    L.B = B;
    L.nblocks = (uint32_t)((n + B - 1) / B);
    L.tpb = (B + kTile - 1) / kTile;
    L.wpb = (B + 63) / 64;
    const uint64_t maxmatch = B / 4;
    L.sstride[0] = round16((B + 7) / 8);                            // literal flags
    L.sstride[1] = round16(B);                                      // chars
    L.sstride[2] = round16((kPBits * maxmatch) / 8 + 1 + 8);        // 11-bit distances
    L.sstride[3] = round16(4 * ((uint64_t)B / 40 + 2) + 16);        // golomb words (<= 0.8 bit/byte)
    L.cpb_total = 0;
    for (uint32_t s = 0; s < kStreams; s++) {
        L.cpb[s] = (L.sstride[s] + kChunk - 1) / kChunk;
        L.cpb_total += L.cpb[s];
    }
    return L;
}
}  // namespace

namespace fcx {
void set_last_error(const std::string &m) { g_err = m; }
}  // namespace fcx

// the match kernel's units (fcx_match.hip under each row of the Makefile's unit table); the values of
// fcx_ctx_match_kernel
enum MatchKernel : int {
    kMatchAuto = -1, kMatchGeneral = 0, kMatchKey4 = 1, kMatchNoFilter = 2, kMatchRuns = 3, kMatchSparse = 4,
    kMatchUniform = 5   // (fcx_ctx_match_kernel only: the uniform unit, fcx_match_uniform.hip, routed calls)
};
// One row per unit: the search units in the order of their route lists (row = list index), then the
// general unit, which has no list.
struct MatchUnit {
    int kernel;            // MatchKernel
    int route;             // its route list (fcx_route_plan.h), -1: none
    int mode;              // the fcx_ctx_set_match_mode number that forces it, and its name there
    const char *label;
    MatchLaunch *launch;
    RestLaunch *rest;      // its looped remainder (routed calls)
};
constexpr MatchUnit kUnits[] = {
    {kMatchSparse, kRouteSparse, 7, "sparse kernel", launch_match_sparse, launch_match_rest_sparse},
    {kMatchRuns, kRouteRuns, 6, "runs kernel", launch_match_runs, launch_match_rest_runs},
    {kMatchKey4, kRouteKey4, 4, "4-byte-key kernel", launch_match_k4, launch_match_rest_k4},
    {kMatchNoFilter, kRouteNoFilter, 5, "no-filter kernel", launch_match_nf, launch_match_rest_nf},
    {kMatchGeneral, -1, 3, "general kernel", launch_match, nullptr},
};
constexpr int kNumUnits = sizeof(kUnits) / sizeof(kUnits[0]);
static_assert(kUnits[kRouteSparse].route == kRouteSparse && kUnits[kRouteRuns].route == kRouteRuns &&
              kUnits[kRouteKey4].route == kRouteKey4 && kUnits[kRouteNoFilter].route == kRouteNoFilter &&
              kNumUnits == kSearchUnits + 1, "kUnits: row = route list");
static const MatchUnit &match_unit(int kernel) {   // (auto: the general unit; its routed calls go by list)
    for (const MatchUnit &u : kUnits)
        if (u.kernel == kernel) return u;
    return kUnits[kSearchUnits];
}
constexpr uint32_t kRestGrid = 512;         // k_match_rest_<unit>'s workgroups (2 per CU: <= 128 VGPRs)
constexpr uint64_t kRouteBytes = 4ull * kRouteWords;       // the route counters of a call
constexpr uint64_t kWordBytes = kCwRouteBytes + kRouteBytes;   // dev_words (the status words of fcx_device.h)
constexpr uint64_t kHwColdBytes = kWordBytes;              // host_words only: byte offset of the first call's counts

// the scratch of a context, sized for cap_n shard bytes; ensure_scratch drops it as a whole
struct CtxScratch {
    uint64_t cap_n = 0;        // shard bytes the scratch is sized for
    uint32_t cap_blocks = 0;
    uint64_t cap_tiles = 0;
    DevBuf<uint32_t> m;
    DevBuf<uint64_t> chain;
    DevBuf<uint64_t> mbits;            // per position: m[] stored (match or unknown)
    DevBuf<uint64_t> chain_pfx;        // per 64 positions: speculative prefix counts (k_match)
    DevBuf<uint32_t> tinfo;            // per tile: flags, exit, token/match/golomb-bit totals
    DevBuf<uint32_t> tile_off;         // per tile: token/match/golomb-bit offsets (k_stitch)
    DevBuf<uint32_t> mtok;             // per tile: compact match list of the speculative chain (k_match)
    DevBuf<uint32_t> tconv;            // per tile: where the final chain joins it (k_resolve / k_stitch)
    DevBuf<uint64_t> fp;               // per tile: fast-path record (k_resolve)
    DevBuf<BlockInfo> binfo;
    DevBuf<uint8_t> s[kStreams];
    DevBuf<uint16_t> thist;            // per tile: chars counts (k_emit)
    DevBuf<uint64_t> cstat;            // per chunk: k_encode's look-back status word
    DevBuf<uint32_t> sdesc;            // per 64 chars: run of input bytes (offset) or kCdMixed (k_emit)
    DevBuf<uint32_t> ctab;             // code table
    DevBuf<uint8_t> ltab, hhdr;
    DevBuf<uint64_t> blk_off;
    DevBuf<uint32_t> rlist;            // route lists: kRoutes x cap_tiles tile indices (k_classify)
    DevBuf<uint8_t> tkind;             // per tile: its unit (k_classify)
};

struct fcx_ctx : CtxScratch {
    int device = 0;
    uint32_t B = 0;
    DevBuf<uint64_t> dev_words;        // the status words (fcx_device.h), kWordBytes
    PinnedBuf<uint64_t> host_words;    // their mirror: [kCwTotal, kCwErr] length reads; kCwLazy and the route
                                       // counters of a recent call (copied back asynchronously after every
                                       // routed call); from kHwColdBytes the first call's counts (waited for)
    RouteHint hint;                    // the routed calls' estimate of each unit's share (fcx_route_plan.h)
    uint32_t last_grid[kRoutes] = {};  // the last call's unit grids
    bool last_routed = false, last_cold = false;
    int last_kernel = kMatchGeneral;   // the last call's match kernel (routed: the unit with the largest grid)
    // profiling
    bool profiling = false;
    uint32_t match_mode = 0;   // k_match tile-mode bits (fcx_ctx_set_match_mode)
    int kernel = kMatchAuto;   // match kernel (MatchKernel): auto = chosen per call from the block kinds
    uint32_t emit_dbg = 0;     // k_emit development exits (fcx_debug_emit_bits; output invalid)
    StageTimes times{kNumStages};   // read on the first fcx_ctx_stage query
    Layout last{};
};
static_assert(kNumStages <= StageTimes::kStages, "StageTimes");

namespace {
int ensure_scratch(fcx_ctx *c, uint64_t n) {
    if (n <= c->cap_n) return FCX_OK;
    static_cast<CtxScratch &>(*c) = CtxScratch{};   // (the old scratch goes before the new is made)
    const Layout L = make_layout(n, c->B);
    const uint64_t nb = L.nblocks, nt = (uint64_t)L.nblocks * L.tpb;
    FCX_TRY(c->m.reserve(4ull * nb * c->B, "m"));
    FCX_TRY(c->chain.reserve(8ull * nb * L.wpb, "chain"));
    FCX_TRY(c->mbits.reserve(8ull * nb * L.wpb, "mbits"));
    FCX_TRY(c->chain_pfx.reserve(8ull * (kTile / 64) * nt, "chain_pfx"));
    FCX_TRY(c->tinfo.reserve(32 * nt, "tinfo"));
    FCX_TRY(c->tile_off.reserve(12 * (nt + 1), "tile_off"));   // (+1: k_emit reads tile tix + 1's)
    FCX_TRY(c->mtok.reserve(4ull * kTileMatches * nt + sparse_tail_bytes(nt), "mtok"));   // (+ the sparse unit's tail flags)
    FCX_TRY(c->tconv.reserve(4 * nt, "tconv"));
    FCX_TRY(c->fp.reserve(96 * nt, "fp"));   // 12 u64 per tile (k_resolve record)
    FCX_TRY(c->binfo.reserve(sizeof(BlockInfo) * nb, "binfo"));
    for (uint32_t s = 0; s < kStreams; s++) FCX_TRY(c->s[s].reserve((uint64_t)L.sstride[s] * nb + 64, "stream"));
    FCX_TRY(c->thist.reserve(2ull * 256 * nt, "thist"));
    FCX_TRY(c->cstat.reserve(16ull * L.cpb_total * nb, "cstat"));
    FCX_TRY(c->sdesc.reserve(4ull * ((c->B + kCharSeg - 1) / kCharSeg) * nb, "sdesc"));
    FCX_TRY(c->ctab.reserve(4ull * 256 * kStreams * nb, "ctab"));
    FCX_TRY(c->ltab.reserve(256ull * kStreams * nb, "ltab"));
    FCX_TRY(c->hhdr.reserve((uint64_t)kHuffHdrStride * kStreams * nb, "hhdr"));
    FCX_TRY(c->blk_off.reserve(8 * nb, "blk_off"));
    FCX_TRY(c->rlist.reserve(4ull * kRoutes * nt, "route lists"));
    FCX_TRY(c->tkind.reserve(nt, "tile kinds"));
    c->cap_tiles = nt;
    c->cap_n = (uint64_t)L.nblocks * c->B;
    c->cap_blocks = L.nblocks;
    return FCX_OK;
}

// The routed match stage of a compress call: classify the shard's tiles into the unit lists, then each
// unit over its list with a grid from the estimate (the first call waits for its own counts),
// k_match_rest for the rest.  ev: the stage events of a profiled call, or null (the route stage ends
// at ev[1])
int match_routed(fcx_ctx *c, const MatchArgs &ma, hipStream_t st, hipEvent_t *ev) {
    uint32_t *rc = (uint32_t *)((uint8_t *)c->dev_words.p + kCwRouteBytes);   // the route counters
    const uint32_t stride = (uint32_t)c->cap_tiles, ntg = ma.L.nblocks * ma.L.tpb;
    auto list_of = [&](uint32_t u) { return c->rlist + (uint64_t)u * stride; };
    launch_classify(ma.in, ma.L, c->rlist, stride, rc, c->tkind, st);
    if (ev) FCX_HIP(hipEventRecord(ev[1], st));
    uint64_t est[kRoutes];
    if (!c->hint.have) {
        uint32_t *cold = (uint32_t *)((uint8_t *)c->host_words.p + kHwColdBytes);
        FCX_HIP(hipMemcpyAsync(cold, rc, 4 * kRouteWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        for (uint32_t u = 0; u < kRoutes; u++) est[u] = cold[u];
        c->hint.adopt(cold, 0);   // (no hand-ons yet, no lazy tiles: fix stays 0)
    } else {
        route_estimate(c->hint.cnt, c->hint.valid, ntg, est);
    }
    const RoutePlan plan = plan_route(est, ntg, c->hint.fix != 0);
    // the uniform unit first: the tiles it hands on join the runs list before any runs launch reads it
    launch_match_uniform(ma, list_of(kRouteUniform), rc + kRouteUniform, list_of(kRouteRuns), rc + kRouteRuns,
                         c->tkind, plan.ugrid, st);
    MatchRoute rts[kSearchUnits];   // per unit: its routed form (its remainder's; its launch's unless direct)
    for (uint32_t u : plan.order) {
        const bool direct = plan.grid[u] == kRestDirect;
        MatchRoute &rt = rts[u];
        rt.kind = c->tkind;
        rt.mine = u;
        rt.cnt = rc + u;
        if (!direct) rt.list = list_of(u);
        if (u == kRouteSparse || u == kRouteRuns) {
            rt.defer_list = list_of(kRouteNoFilter);
            rt.defer_cnt = rc + kRouteNoFilter;
        }
        // the no-filter list's length now, before its listed launch (rest_start)
        if (rest_start(plan.grid[u], u).word == (int)kRcCover) launch_route_mark(rc + kRcCover, rc + kRouteNoFilter, st);
        // (direct over every tile: the unrouted code, no kind check and no hand-on)
        const MatchRoute launch = direct && plan.every ? MatchRoute{} : rt;
        kUnits[u].launch(ma, st, 0u, &launch, direct ? 0u : plan.grid[u]);
        c->last_grid[u] = plan.grid[u];
        // the sparse unit's second phase right after a direct launch, which has every tile of its kind:
        // over every tile of the shard it also flagged tiles of other kinds, whose own units search them
        // again below and reuse their mtok slots
        if (u == kRouteSparse && direct) launch_sparse_tail(ma, st);
    }
    c->last_kernel = est[kRouteUniform] > est[plan.best] ? kMatchUniform
                     : est[plan.best]                    ? kUnits[plan.best].kernel
                                                         : kMatchGeneral;
    // each unit's remainder (the no-filter one last: it takes the others' hand-ons); a direct
    // sparse / runs / 4-byte launch leaves none
    for (uint32_t u = 0; u < kSearchUnits; u++) {
        const RestStart rs = rest_start(plan.grid[u], u);
        if (rs.none()) continue;
        const RouteRest rest{list_of(u), rc + u, rs.start, rs.word >= 0 ? rc + rs.word : nullptr};
        kUnits[u].rest(ma, rest, rts[u], kRestGrid, st);
        // (listed, the sparse unit has its own tiles only: one tail launch after its remainder)
        if (u == kRouteSparse) launch_sparse_tail(ma, st);
    }
    return FCX_OK;
}
}  // namespace

extern "C" {

const char *fcx_last_error(void) { return g_err.c_str(); }
const char *fcx_version(void) { return "fcx-mi355x 0.1 (gfx950)"; }

uint64_t fcx_shard_bound(uint64_t n, uint32_t block_bytes) {
    if (block_bytes == 0) return 0;
    const uint64_t nb = (n + block_bytes - 1) / block_bytes;
    // per block: record/stream headers (<= 4 x 580 + 24) + Huffman words (< 2x input)
    return 2 * n + nb * 4096 + 64;
}

int fcx_write_header(uint8_t *out10, uint64_t total_in, uint64_t nblocks) {
    if (!out10) return fail(FCX_ERR_ARG, "fcx_write_header: NULL");
    memcpy(out10, "FCX7", 4);
    const uint32_t t = (uint32_t)total_in;      // cmp_before_bytes wraps (:104)
    const uint16_t nb = (uint16_t)nblocks;      // block_num is u16 (:105)
    memcpy(out10 + 4, &t, 4);
    memcpy(out10 + 8, &nb, 2);
    return FCX_OK;
}

int fcx_parse_header(const uint8_t *in10, uint32_t *total_in, uint16_t *nblocks, char *kind) {
    if (!in10) return fail(FCX_ERR_ARG, "fcx_parse_header: NULL");
    if (memcmp(in10, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream (:4147)");
    if (total_in) memcpy(total_in, in10 + 4, 4);
    if (nblocks) memcpy(nblocks, in10 + 8, 2);
    if (kind) *kind = (char)in10[3];
    return FCX_OK;
}

int fcx_ctx_create(fcx_ctx **out, int device, uint32_t block_bytes, uint64_t max_shard_bytes) {
    if (!out) return fail(FCX_ERR_ARG, "fcx_ctx_create: NULL ctx");
    *out = nullptr;
    if (block_bytes == 0 || block_bytes > FCX_MAX_BLOCK_BYTES)
        return fail(FCX_ERR_ARG, "block_bytes must be in [1, 1 MiB] (reference decoder limit :2373)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(FCX_ERR_HIP, "no HIP device: the compress path is GPU-only");
    if (device < 0 || device >= ndev) return fail(FCX_ERR_ARG, "bad device index");
    FCX_HIP(hipSetDevice(device));
    std::unique_ptr<fcx_ctx, Calls<fcx_ctx_destroy>> c(new fcx_ctx());
    c->device = device;
    c->B = block_bytes;
    if ((e = c->host_words.alloc(kHwColdBytes + kRouteBytes)) != hipSuccess)
        return fail(FCX_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    memset(c->host_words, 0, kHwColdBytes + kRouteBytes);
    if ((e = c->dev_words.alloc(kWordBytes)) != hipSuccess)
        return fail(FCX_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    FCX_TRY(ensure_scratch(c.get(), max_shard_bytes ? max_shard_bytes : block_bytes));
    *out = c.release();
    return FCX_OK;
}

void fcx_ctx_destroy(fcx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
}

const uint64_t *fcx_ctx_device_out_len(fcx_ctx *c) { return c ? c->dev_words.p : nullptr; }

namespace {
// the verdict of a call's error bits (host_words after a length read)
int check_err_bits(const fcx_ctx *c) {
    const uint32_t e = (uint32_t)c->host_words[kCwErr];
    if (e & kErrCapacity) return fail(FCX_ERR_CAPACITY, "output capacity too small (see fcx_shard_bound)");
    if (e) return fail(FCX_ERR_INTERNAL, "device invariant violated (error bits " + std::to_string(e) + ")");
    return FCX_OK;
}
}  // namespace

int fcx_ctx_read_out_len(fcx_ctx *c, uint64_t *out_len) {
    if (!c || !out_len) return fail(FCX_ERR_ARG, "fcx_ctx_read_out_len: NULL");
    FCX_HIP(hipSetDevice(c->device));
    FCX_HIP(hipDeviceSynchronize());
    FCX_HIP(hipMemcpy(c->host_words, c->dev_words, kCwHeadBytes, hipMemcpyDeviceToHost));
    FCX_TRY(check_err_bits(c));
    *out_len = c->host_words[kCwTotal];
    return FCX_OK;
}

int fcx_ctx_set_profiling(fcx_ctx *c, int enable) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    c->profiling = enable != 0;
    return FCX_OK;
}

int fcx_ctx_set_match_mode(fcx_ctx *c, int mode) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    // 0: routed; 1-2: the general unit under k_match dbg bits (all keep the output exact); from 3: a unit
    int kernel = mode == 0 ? kMatchAuto : kMatchGeneral;
    bool known = mode >= 0 && mode <= 2;
    for (const MatchUnit &u : kUnits)
        if (u.mode == mode) { kernel = u.kernel; known = true; }
    if (!known) {
        std::string msg = "match mode must be 0 (auto), 1 (bucket search), 2 (run table)";
        for (int q = 3; q < 3 + kNumUnits; q++)   // (the units' numbers follow 2 without a gap)
            for (const MatchUnit &u : kUnits)
                if (u.mode == q) msg += (q == 2 + kNumUnits ? " or " : ", ") + std::to_string(q) + " (" + u.label + ")";
        return fail(FCX_ERR_ARG, msg);
    }
    c->match_mode = mode == 1 ? 4u | 128u : mode == 2 ? 8u : 0u;
    c->kernel = kernel;
    return FCX_OK;
}

int fcx_ctx_stage_count(fcx_ctx *c) { return c ? c->times.n : 0; }

int fcx_ctx_stage(fcx_ctx *c, int i, const char **name, float *ms) {
    if (!c || i < 0 || i >= kNumStages) return fail(FCX_ERR_ARG, "bad stage");
    if (!c->times.n) return fail(FCX_ERR_ARG, "last call was not profiled");
    return c->times.stage(i, name, ms);
}

int fcx_compress_shard(fcx_ctx *c, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap,
                       uint64_t *out_len, void *stream) {
    if (!c || !d_out || (n && !d_in)) return fail(FCX_ERR_ARG, "fcx_compress_shard: NULL argument");
    if (((uintptr_t)d_out & 15) != 0) return fail(FCX_ERR_ARG, "d_out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    FCX_HIP(hipSetDevice(c->device));
    if (n == 0) {
        FCX_HIP(hipMemsetAsync(c->dev_words, 0, kCwHeadBytes, st));
        if (out_len) *out_len = 0;
        return FCX_OK;
    }
    if (n / c->B >= 65536 * 2048ull) return fail(FCX_ERR_ARG, "shard too large");
    FCX_TRY(ensure_scratch(c, n));
    const Layout L = make_layout(n, c->B);
    c->last = L;
    uint64_t *total = c->dev_words + kCwTotal;
    uint32_t *err = (uint32_t *)(c->dev_words + kCwErr);
    c->times.reset();
    hipEvent_t *ev = nullptr;   // the stage events of a profiled call
    if (c->profiling) {
        c->times.publish(kStageNames, kNumStages, true);
        ev = c->times.events();
    }

    // match search: unrouted when a unit is forced (fcx_ctx_set_match_mode), else routed per tile
    // (fcx_route.hip): the estimates of each unit's share come from the route counters of a recent
    // call (landing asynchronously: any values are a valid estimate, they only size the grids)
    const bool routed = c->kernel == kMatchAuto;
    if (routed && c->hint.have) {
        const uint32_t *hr = (const uint32_t *)((const uint8_t *)c->host_words.p + kCwRouteBytes);
        uint32_t counters[kRouteWords];
        for (uint32_t w = 0; w < kRouteWords; w++) counters[w] = __atomic_load_n(&hr[w], __ATOMIC_RELAXED);
        const uint32_t lazy = (uint32_t)__atomic_load_n(&c->host_words[kCwLazy], __ATOMIC_RELAXED);   // (k_tree)
        c->hint.adopt(counters, lazy);
    }
    c->last_routed = routed;
    c->last_cold = routed && !c->hint.have;
    c->last_kernel = routed ? kMatchGeneral : c->kernel;
    FCX_HIP(hipMemsetAsync(c->dev_words, 0, kWordBytes, st));
    const MatchArgs ma{d_in, L, c->m, c->mbits, c->chain, c->chain_pfx, c->tinfo, c->mtok};
    const bool tail = routed || c->kernel == kMatchSparse;   // the sparse unit may run: its tail flags start clear
    if (tail) FCX_HIP(hipMemsetAsync(sparse_tail_head(ma.mtok, L.nblocks * L.tpb), 0, sparse_tail_flag_bytes(L.nblocks * L.tpb), st));
    if (ev) FCX_HIP(hipEventRecord(ev[0], st));   // (the memsets above are not timed)
    if (!routed) {
        if (ev) FCX_HIP(hipEventRecord(ev[1], st));
        match_unit(c->kernel).launch(ma, st, c->match_mode, nullptr, 0);
        if (tail) launch_sparse_tail(ma, st);
    } else {
        FCX_TRY(match_routed(c, ma, st, ev));
    }
    if (ev) FCX_HIP(hipEventRecord(ev[2], st));
    launch_parse(d_in, L, ma.m, ma.mbits, ma.chain, ma.chain_pfx, ma.tinfo, ma.mtok, c->fp, c->tile_off, c->tconv,
                 c->binfo, c->s[0], c->s[1], c->s[2], c->s[3], c->thist, c->sdesc, err, st, ev ? ev + 3 : nullptr,
                 c->emit_dbg);
    if (c->emit_dbg & 0xFFFFu) {   // (development: k_emit's timing exits leave invalid streams; stop here)
        if (ev)
            for (int q = 5; q <= kNumStages; q++) FCX_HIP(hipEventRecord(ev[q], st));
    } else {
        launch_entropy(L, c->binfo, c->s[0], c->s[1], c->s[2], c->s[3], c->thist, c->ctab, c->ltab, c->hhdr, c->cstat,
                       c->blk_off, total, d_out, cap, err, d_in, c->sdesc, st, ev ? ev + 5 : nullptr, c->emit_dbg >> 16);
    }
    FCX_HIP(hipGetLastError());
    if (routed) {   // the lazy tiles and route counters back for the next calls' estimates (asynchronous)
        FCX_HIP(hipMemcpyAsync(c->host_words + kCwLazy, c->dev_words + kCwLazy, kWordBytes - 8 * kCwLazy,
                               hipMemcpyDeviceToHost, st));
        c->hint.have = true;
    }
    if (out_len) {
        FCX_HIP(hipMemcpyAsync(c->host_words, c->dev_words, kCwHeadBytes, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        FCX_TRY(check_err_bits(c));
        *out_len = c->host_words[kCwTotal];
    }
    return FCX_OK;
}

int fcx_ctx_stats(fcx_ctx *c, uint64_t *tokens, uint64_t *matches, uint64_t *lazy_evals, uint64_t *lazy_tiles,
                  uint64_t *tiles) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    const uint32_t nb = c->last.nblocks;
    std::vector<BlockInfo> bi(nb);
    FCX_HIP(hipSetDevice(c->device));
    FCX_HIP(hipDeviceSynchronize());
    if (nb) FCX_HIP(hipMemcpy(bi.data(), c->binfo, sizeof(BlockInfo) * nb, hipMemcpyDeviceToHost));
    uint64_t t = 0, mt = 0, le = 0, lt = 0;
    for (auto &x : bi) { t += x.ntok; mt += x.nmatch; le += x.lazy_evals; lt += x.lazy_tiles; }
    if (tokens) *tokens = t;
    if (matches) *matches = mt;
    if (lazy_evals) *lazy_evals = le;
    if (lazy_tiles) *lazy_tiles = lt;
    if (tiles) {
        uint64_t tl = 0;
        for (auto &x : bi) tl += (x.len + kTile - 1) / kTile;
        *tiles = tl;
    }
    return FCX_OK;
}

// development only (not in fcx.h): k_emit's (bits 0..15) and k_tree's (bits 16..) timing exits for the
// following compress calls (their output is invalid while bits are set; 0 restores the product kernels)
int fcx_debug_emit_bits(fcx_ctx *c, uint32_t bits) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    c->emit_dbg = bits;
    return FCX_OK;
}

int fcx_ctx_match_kernel(fcx_ctx *c) { return c ? c->last_kernel : -1; }

int fcx_ctx_route_stats(fcx_ctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_ctx_route_stats: bad argument");
    uint64_t v[FCX_ROUTE_STATS] = {};
    if (c->last_routed) {
        FCX_HIP(hipSetDevice(c->device));
        FCX_HIP(hipDeviceSynchronize());
        uint32_t r[kRouteWords];
        FCX_HIP(hipMemcpy(r, (uint8_t *)c->dev_words.p + kCwRouteBytes, sizeof(r), hipMemcpyDeviceToHost));
        for (uint32_t u = 0; u < kSearchUnits; u++) {
            v[u] = r[u];
            const uint32_t s0 = rest_start(c->last_grid[u], u, r);
            v[6] += r[u] > s0 ? r[u] - s0 : 0u;
        }
        v[4] = r[kRouteNoFilter] - r[kRcNfFiled] + r[kRouteRuns] - r[kRcRunsFiled];
        v[5] = r[kRcValid];
        v[7] = c->last_cold;
        v[8] = r[kRouteUniform];
    }
    for (int i = 0; i < n && i < FCX_ROUTE_STATS; i++) out[i] = v[i];
    return c->last_routed ? FCX_OK : fail(FCX_ERR_ARG, "the last call was not routed (a match unit is forced)");
}

// development only (not in fcx.h): the match kernel alone with experiment bits, for
// per-phase timing (tools/matchphase.py); the context's scratch is left invalid
int fcx_debug_match(fcx_ctx *c, const uint8_t *d_in, uint64_t n, uint32_t dbg, void *stream) {
    if (!c || !d_in || n == 0) return fail(FCX_ERR_ARG, "fcx_debug_match: bad argument");
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ensure_scratch(c, n));
    const MatchArgs ma{d_in, make_layout(n, c->B), c->m, c->mbits, c->chain, c->chain_pfx, c->tinfo, c->mtok};
    // the sparse unit: its tail kernel follows unless the bits end the kernel at a phase (16, 4096, 32:
    // staging, filter, search; 64: the end of phase 1, the tail flags written; 256-2048, 8192: the
    // parse's and the run table's exits).  Bit 131072 keeps every tile's queries in the workgroup.
    const bool tail = c->kernel == kMatchSparse;
    if (tail)
        FCX_HIP(hipMemsetAsync(sparse_tail_head(ma.mtok, ma.L.nblocks * ma.L.tpb), 0,
                               sparse_tail_flag_bytes(ma.L.nblocks * ma.L.tpb), (hipStream_t)stream));
    match_unit(c->kernel).launch(ma, (hipStream_t)stream, dbg, nullptr, 0);
    if (tail && !(dbg & (16u | 32u | 64u | 256u | 512u | 1024u | 2048u | 4096u | 8192u)))
        launch_sparse_tail(ma, (hipStream_t)stream);
    FCX_HIP(hipGetLastError());
    return FCX_OK;
}

// development only (not in fcx.h): the tiles of the last compress call that k_match_sparse left to its
// tail kernel (the tail list's length; 0 when the sparse unit did not run)
int fcx_debug_sparse_tail_count(fcx_ctx *c, uint64_t *listed) {
    if (!c || !listed) return fail(FCX_ERR_ARG, "fcx_debug_sparse_tail_count: NULL");
    *listed = 0;
    if (!c->last.nblocks || !(c->last_routed || c->last_kernel == kMatchSparse)) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_HIP(hipDeviceSynchronize());
    uint32_t n = 0;
    FCX_HIP(hipMemcpy(&n, sparse_tail_head(c->mtok, c->last.nblocks * c->last.tpb), 4, hipMemcpyDeviceToHost));
    *listed = n;
    return FCX_OK;
}

// development only (not in fcx.h): the routed call's launch plan (fcx_route_plan.h) for the tests; no GPU.
// out: ugrid, best, direct, every, order[4], grid[4]
int fcx_debug_route_plan(const uint64_t est[5], uint32_t ntg, int fix, uint32_t out[12]) {
    if (!est || !out) return fail(FCX_ERR_ARG, "fcx_debug_route_plan: NULL");
    const RoutePlan p = plan_route(est, ntg, fix != 0);
    out[0] = p.ugrid; out[1] = p.best; out[2] = p.direct; out[3] = p.every;
    for (uint32_t u = 0; u < kSearchUnits; u++) { out[4 + u] = p.order[u]; out[8 + u] = p.grid[u]; }
    return FCX_OK;
}
// ... its estimates from a recent call's counts (est[5]) ...
int fcx_debug_route_estimate(const uint64_t cnt[5], uint64_t valid, uint32_t ntg, uint64_t est[5]) {
    if (!cnt || !est) return fail(FCX_ERR_ARG, "fcx_debug_route_estimate: NULL");
    route_estimate(cnt, valid, ntg, est);
    return FCX_OK;
}
// ... and where a unit's remainder starts, given its grid in the plan and the call's 16 route counters
uint32_t fcx_debug_rest_start(uint32_t grid, uint32_t unit, const uint32_t counters[16]) {
    return unit < kSearchUnits && counters ? rest_start(grid, unit, counters) : ~0u;
}
// ... and the estimate a context keeps (RouteHint) after it adopts a call's 16 route counters and lazy
// tiles.  hint: cnt[5], valid, fix, in and out
int fcx_debug_route_hint(uint64_t hint[7], const uint32_t counters[16], uint32_t lazy) {
    if (!hint || !counters) return fail(FCX_ERR_ARG, "fcx_debug_route_hint: NULL");
    RouteHint h;
    for (uint32_t u = 0; u < kRoutes; u++) h.cnt[u] = hint[u];
    h.valid = hint[5];
    h.fix = hint[6];
    h.adopt(counters, lazy);
    for (uint32_t u = 0; u < kRoutes; u++) hint[u] = h.cnt[u];
    hint[5] = h.valid;
    hint[6] = h.fix;
    return FCX_OK;
}

// development only (not in fcx.h): the sparse unit's repeat filter on the host (fcx_sparse_filter.h), for
// the tests; no GPU.  The 3-byte keys at positions 0 .. nkeys - 1 of win (nkeys + 2 bytes) are inserted
// in position order into an empty bitmap; flags (may be NULL): 1 per flagged position.
// out: flagged count, the flagged-key cap, R's capacity, bits per key
int fcx_debug_sparse_filter(const uint8_t *win, uint32_t nkeys, uint8_t *flags, uint32_t out[4]) {
    if (!win || !out) return fail(FCX_ERR_ARG, "fcx_debug_sparse_filter: NULL");
    std::vector<uint32_t> bm(kSfWords, 0u);
    uint32_t nflag = 0;
    for (uint32_t x = 0; x < nkeys; x++) {
        const uint32_t key = (uint32_t)win[x] | ((uint32_t)win[x + 1] << 8) | ((uint32_t)win[x + 2] << 16);
        const uint32_t bits = sf_bits(key);
        uint32_t &w = bm[sf_word(key)];
        const bool flagged = (w & bits) == bits;
        w |= bits;
        nflag += flagged;
        if (flags) flags[x] = flagged;
    }
    out[0] = nflag; out[1] = kSfFlagCap; out[2] = kSfRCap; out[3] = kSfK;
    return FCX_OK;
}

int fcx_ctx_info(fcx_ctx *c, int *device, uint32_t *block_bytes, uint64_t *shard_bytes) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    if (device) *device = c->device;
    if (block_bytes) *block_bytes = c->B;
    if (shard_bytes) *shard_bytes = c->cap_n ? c->cap_n : c->B;
    return FCX_OK;
}

uint32_t fcx_compress_block(const void *in, uint32_t len, uint8_t *out) {
    if (!in || !out) return 0;  // :2122-2123
    if (len == 0) {
        // the reference's encoding of an empty block (2115-2253 with totalBytes = 0): u32 N = 0,
        // no flag bytes (nb = 0) and no chars HUFF (charNum = 0, 989-990), u32 pCnt = 0, HUFF
        // of the one zero byte of the (11*0)/8+1-byte distance buffer (ts = 0, W = 0: 5 bytes),
        // u32 G = 0 -- 17 zero bytes, pinned by golden.json kat["empty_block"]
        memset(out, 0, 17);
        return 17;
    }
    if (len > FCX_MAX_BLOCK_BYTES) { fail(FCX_ERR_ARG, "block larger than 1 MiB"); return 0; }
    // a context per host thread, on the device that was current at the thread's first call
    thread_local std::unique_ptr<fcx_ctx, Calls<fcx_ctx_destroy>> ctx;
    thread_local std::vector<uint8_t> buf;
    if (!ctx) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        fcx_ctx *c = nullptr;
        if (fcx_ctx_create(&c, dev, FCX_MAX_BLOCK_BYTES, FCX_MAX_BLOCK_BYTES)) return 0;
        ctx.reset(c);
    }
    buf.resize(fcx_shard_bound(len, FCX_MAX_BLOCK_BYTES));
    uint64_t got = 0;
    if (fcx_compress_host(ctx.get(), (const uint8_t *)in, len, buf.data(), buf.size(), &got)) return 0;
    if (got < 4) { fail(FCX_ERR_INTERNAL, "short record"); return 0; }
    uint32_t plen;
    memcpy(&plen, buf.data(), 4);
    memcpy(out, buf.data() + 4, plen);
    return plen;
}

}  // extern "C"
