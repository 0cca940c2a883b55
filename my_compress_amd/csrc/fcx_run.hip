// fcx_run.hip — the run core: the host half of every call over a device-resident run of
// FCX7 / FCX8 records that is indexed, decoded group by group into the verification's bounded buffer and
// judged block by block: verify_run (fcx_verify.hip), repair_apply_run (fcx_repair.hip) and check_run
// (fcx_digest.hip); or searched or counted across the blocks: find_run (fcx_find.hip), lines_run (fcx_lines.hip).  Host code only; the stage times of such a call: RunTimes (fcx_dec_shared.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"

namespace fcx {

constexpr uint32_t kVGroupRecords = 1u << 20;     // records per group at most (the grid)
constexpr uint64_t kVGroupBytes = 256ull << 20;   // decoded bytes per group by default

// groups of consecutive records whose decoded bytes fit the bound, a record of no bytes counted
// as one (so a bound of 1 makes every record a group); a record larger than the bound is a group
// of its own.  doff: the run's dec_off on the host; returns the end of the group that starts at g0.
uint32_t verify_group_end(const VerifyScratch &V, const uint64_t *doff, uint32_t nblocks, uint32_t g0) {
    const uint64_t bound = V.group_bytes ? V.group_bytes : kVGroupBytes;
    uint32_t g1 = g0;
    uint64_t cost = 0;
    do {
        cost += std::max<uint64_t>(doff[g1 + 1] - doff[g1], 1);
        g1++;
    } while (g1 < nblocks && g1 - g0 < kVGroupRecords && cost + std::max<uint64_t>(doff[g1 + 1] - doff[g1], 1) <= bound);
    return g1;
}

int run_args(const char *fn, fcx_dctx *c, char kind, const void *d_rec, uint32_t nblocks, uint64_t n, uint32_t B) {
    const std::string f(fn);
    if (!c) return fail(FCX_ERR_ARG, f + ": NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, f + ": kind must be '7' or '8'");
    if (B == 0 || B > FCX_MAX_BLOCK_BYTES) return fail(FCX_ERR_ARG, f + ": block_bytes outside [1, FCX_MAX_BLOCK_BYTES]");
    if ((n + B - 1) / B != nblocks) return fail(FCX_ERR_ARG, f + ": nblocks is not ceil(n / block_bytes)");
    if (nblocks && !d_rec) return fail(FCX_ERR_ARG, f + ": NULL argument");
    return FCX_OK;
}

int run_index(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, hipStream_t st, RunTimes &T,
              RunIndex *ix) {
    RangeScratch &R = c->rg;   // the index of the run, in the range API's scratch
    FCX_TRY(R.rec_off.reserve(8ull * nblocks + 8, "index"));
    FCX_TRY(R.dec_off.reserve(8ull * nblocks + 8, "index"));
    T.mark(0);
    FCX_TRY(fcx_index_shard(c, kind, d_rec, rec_len, nblocks, R.rec_off, R.dec_off, nullptr, st));
    T.mark(1);
    ix->roff.resize(nblocks + 1);
    ix->doff.resize(nblocks + 1);
    FCX_HIP(hipMemcpyAsync(ix->roff.data(), R.rec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemcpyAsync(ix->doff.data(), R.dec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    return FCX_OK;
}

int run_groups(fcx_dctx *c, const RunIndex &ix, uint32_t nblocks, std::vector<RunGroup> *groups,
               const std::function<bool(uint32_t, uint32_t)> &staged, uint64_t headroom) {
    VerifyScratch &V = c->vf;
    const uint64_t *doff = ix.doff.data();
    uint64_t need = 0;
    groups->clear();
    for (uint32_t g0 = 0; g0 < nblocks;) {
        const uint32_t g1 = verify_group_end(V, doff, nblocks, g0);
        groups->push_back({g0, g1, doff[g1] - doff[g0]});
        if (!staged || staged(g0, g1)) need = std::max(need, doff[g1] - doff[g0]);
        g0 = g1;
    }
    V.groups = (uint32_t)groups->size();
    return V.buf.reserve(need + headroom + 64, "verify buffer");
}

int decode_group(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, const std::vector<uint64_t> &roff, uint32_t g0,
                 uint32_t nrec, uint8_t *dst, uint64_t want, hipStream_t st, uint64_t rec_base, const char *who) {
    // (an index entry can only lie inside the run: the index was built from it just now)
    const uint64_t at = roff[g0];
    uint64_t got = 0;
    if (kind == '7') FCX_TRY(fcx_decompress_shard(c, d_rec + at, rec_len - at, nrec, dst, want, &got, st));
    else FCX_TRY(lz78_decompress_shard_at(c, d_rec + at, rec_len - at, nrec, dst, want, &got, st, rec_base + g0));
    if (got != want) return fail(FCX_ERR_INTERNAL, std::string(who) + ": the decode of a group disagrees with the index");
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_dctx_set_verify_group(fcx_dctx *c, uint64_t bytes) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    c->vf.group_bytes = bytes;
    return FCX_OK;
}

int fcx_dctx_verify_groups(fcx_dctx *c) { return c ? (int)c->vf.groups : -1; }

}  // extern "C"
