// fcx_verify.hip — round-trip verification of a device-resident run of FCX7 / FCX8 records against
// the bytes that were compressed (gfx950): fcx_verify_shard of include/fcx.h.  DESIGN.md §9d.
//
// The format is not lossless for every input (the FCX7 early stop, one-symbol sub-streams, the FCX8
// tail-zero rule), so the question "does record k decode back to block k" needs the decoders:
//
//   index        fcx_index_shard: rec_off and dec_off of every record (the size pass);
//   groups       consecutive records whose decoded bytes fit the context's bounded buffer, each
//                through the full decoder entry on the sub-run d_rec + rec_off[g0];
//   k_vcompare   per group: decoded block k against original block k, 16 bytes per lane and step,
//                the first differing byte of a block by atomicMin into first_diff[k];
//   k_vsummary   one workgroup: the size rule folded in, the (decoded, first difference) pairs and
//                the six totals.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_device.h"   // wave_max_dpp, wave_sum_u64
#include "fcx_ld16.h"     // ld16_shifted

namespace fcx {

constexpr uint32_t kVThreads = 256;
constexpr uint32_t kVChunk = 16384;                       // bytes of a block one workgroup compares
constexpr uint32_t kVSteps = kVChunk / (16 * kVThreads);  // 16-byte pieces per lane
constexpr uint32_t kVGroupRecords = 1u << 20;             // records per group at most (the grid)
constexpr uint64_t kVGroupBytes = 256ull << 20;           // decoded bytes per group by default

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

// minimum over the 64 lanes (uniform); every lane of the wave must be active
__device__ inline uint32_t wave_min_dpp(uint32_t v) { return ~wave_max_dpp(~v); }

// index of the first differing byte of two 16-byte pieces, 16 if none
__device__ inline uint32_t first_diff16(uint4 a, uint4 b) {
    const uint32_t x0 = a.x ^ b.x, x1 = a.y ^ b.y, x2 = a.z ^ b.z, x3 = a.w ^ b.w;
    if (x0) return (uint32_t)__builtin_ctz(x0) >> 3;
    if (x1) return 4 + ((uint32_t)__builtin_ctz(x1) >> 3);
    if (x2) return 8 + ((uint32_t)__builtin_ctz(x2) >> 3);
    if (x3) return 12 + ((uint32_t)__builtin_ctz(x3) >> 3);
    return 16;
}

// Records [k0, k0 + nrec) of the run, decoded back to back at dec (the group's buffer: byte 0 is
// decoded offset dec_base of the run), against their blocks of the original.  Workgroup (chunk c of
// record r): bytes [c kVChunk, (c + 1) kVChunk) of the common prefix of decoded record and original
// block.  Both sides start anywhere: the block at k B for any B, the record at dec_off[k].  A piece
// whose aligned 32-byte window lies inside the block on both sides takes the 16-byte loads; the
// pieces at a block's head and tail go byte by byte, so nothing outside a block is read on either
// side (the original ends at d_orig + n, the decoded bytes at the group's).
__global__ __launch_bounds__(kVThreads) void k_vcompare(const uint8_t *__restrict__ dec, uint64_t dec_base,
                                                        const uint64_t *__restrict__ dec_off, uint32_t k0, uint32_t cpb,
                                                        const uint8_t *__restrict__ orig, uint64_t n, uint32_t B,
                                                        uint32_t *__restrict__ first_diff) {
    const uint32_t k = k0 + blockIdx.x / cpb, c = blockIdx.x % cpb;
    const uint64_t o0 = (uint64_t)k * B, d0 = dec_off[k];
    const uint32_t blen = o0 < n ? (uint32_t)min((uint64_t)B, n - o0) : 0u;
    const uint32_t dlen = (uint32_t)(dec_off[k + 1] - d0);
    const uint32_t m = min(blen, dlen);
    if ((uint64_t)c * kVChunk >= m) return;   // (the whole workgroup)
    const uint8_t *pa = orig + o0, *pb = dec + (d0 - dec_base);
    const uint32_t sa = (uint32_t)((uintptr_t)pa & 15), sb = (uint32_t)((uintptr_t)pb & 15);
    uint32_t best = FCX_VERIFY_SAME;
#pragma unroll
    for (uint32_t s = 0; s < kVSteps; s++) {
        const uint32_t i = c * kVChunk + 16 * (s * kVThreads + threadIdx.x);
        if (i >= m) continue;
        // inside: the aligned windows [i - sh, i - sh + 32) within [0, len) on both sides
        const bool wide = i >= sa && i >= sb && i - sa + 32 <= blen && i - sb + 32 <= dlen;
        uint32_t f = 16;
        if (wide) {
            f = first_diff16(ld16_shifted(pa + i, sa), ld16_shifted(pb + i, sb));
        } else {
            const uint32_t e = min(16u, m - i);
            for (uint32_t j = e; j-- > 0;)
                if (pa[i + j] != pb[i + j]) f = j;
        }
        if (f < 16) best = min(best, i + f);
    }
    best = wave_min_dpp(best);
    if ((threadIdx.x & 63) == 0 && best != FCX_VERIFY_SAME) atomicMin(first_diff + k, best);
}

// One workgroup over the nblocks records: the size rule folded into first_diff (no differing byte in
// the common prefix but sizes that differ: the prefix's length; a record the original has no bytes
// for differs at 0), the pairs (decoded bytes, first difference) to blocks (may be null), and the
// totals into the status words (kVw*, zeroed before, kVwFirst preset to ~0).
__global__ __launch_bounds__(1024) void k_vsummary(uint32_t nblocks, const uint64_t *__restrict__ dec_off, uint64_t n,
                                                   uint32_t B, const uint32_t *__restrict__ first_diff,
                                                   uint32_t *__restrict__ blocks, uint64_t *__restrict__ words) {
    uint64_t differ = 0, first = ~0ull, sized = 0, bytes = 0;
    for (uint32_t k = threadIdx.x; k < nblocks; k += 1024) {
        const uint64_t o0 = (uint64_t)k * B;
        const uint32_t blen = o0 < n ? (uint32_t)min((uint64_t)B, n - o0) : 0u;
        const uint32_t dlen = (uint32_t)(dec_off[k + 1] - dec_off[k]);
        uint32_t fd = first_diff[k];
        if (fd == FCX_VERIFY_SAME && dlen != blen) fd = min(dlen, blen);
        if (o0 >= n) fd = 0;
        if (blocks) {
            blocks[2 * k] = dlen;
            blocks[2 * k + 1] = fd;
        }
        if (dlen != blen) sized++;
        if (fd != FCX_VERIFY_SAME) {
            differ++;
            bytes += blen;
            first = min(first, (uint64_t)k);
        }
    }
    differ = wave_sum_u64(differ);
    sized = wave_sum_u64(sized);
    bytes = wave_sum_u64(bytes);
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)first, o, 64), hi = __shfl_xor((uint32_t)(first >> 32), o, 64);
        first = min(first, ((uint64_t)hi << 32) | lo);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *w = (unsigned long long *)words;
        if (differ) {
            atomicAdd(w + kVwDiffer, (unsigned long long)differ);
            atomicAdd(w + kVwBytes, (unsigned long long)bytes);
            atomicMin(w + kVwFirst, (unsigned long long)first);
        }
        if (sized) atomicAdd(w + kVwSized, (unsigned long long)sized);
    }
    if (threadIdx.x == 0) {
        words[kVwBlocks] = nblocks;
        words[kVwDecoded] = dec_off[nblocks];
    }
}

namespace {
const char *kVStageNames[] = {"index", "decode", "compare", "summary"};
constexpr int kVStages = 4;
}  // namespace

// fcx_verify_shard behind its argument checks, also for the stream path's groups of a longer file:
// nblocks may exceed ceil(n / block_bytes) (records the original has no bytes for: they differ, with
// block length 0), and messages number the records from rec_base.
int verify_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *d_orig,
               uint64_t n, uint32_t B, uint32_t *d_blocks, uint64_t *stats, hipStream_t st, uint64_t rec_base) {
    for (int i = 0; i < FCX_VERIFY_STATS; i++) stats[i] = 0;
    stats[kVwFirst] = ~0ull;
    if (nblocks == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    VerifyScratch &V = c->vf;
    RangeScratch &R = c->rg;
    if (!V.host_words) {
        FCX_TRY(V.words.reserve(8 * kVwWords, "verify words"));
        FCX_HIP(V.host_words.alloc(8 * kVwWords));
    }
    const bool prof = c->profiling;
    std::unique_ptr<StageTimes> T(prof ? new StageTimes(kVStages) : nullptr);
    auto mark = [&](int i) { if (prof) T->mark(i, st); };
    // the index of the run, in the range API's scratch, and a copy of it for the grouping
    FCX_TRY(R.rec_off.reserve(8ull * nblocks + 8, "index"));
    FCX_TRY(R.dec_off.reserve(8ull * nblocks + 8, "index"));
    FCX_TRY(V.first_diff.reserve(4ull * nblocks, "first differences"));
    mark(0);
    FCX_TRY(fcx_index_shard(c, kind, d_rec, rec_len, nblocks, R.rec_off, R.dec_off, nullptr, st));
    mark(1);
    if (prof) FCX_TRY(T->add(0, 1));
    std::vector<uint64_t> roff(nblocks + 1), doff(nblocks + 1);
    FCX_HIP(hipMemcpyAsync(roff.data(), R.rec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemcpyAsync(doff.data(), R.dec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemsetAsync(V.first_diff, 0xFF, 4ull * nblocks, st));
    FCX_HIP(hipMemsetAsync(V.words, 0, 8 * kVwWords, st));
    FCX_HIP(hipMemsetAsync(V.words + kVwFirst, 0xFF, 8, st));
    FCX_HIP(hipStreamSynchronize(st));
    auto group_end = [&](uint32_t g0) { return verify_group_end(V, doff.data(), nblocks, g0); };
    uint64_t need = 0;
    uint32_t ngroups = 0;
    for (uint32_t g0 = 0; g0 < nblocks; g0 = group_end(g0), ngroups++) need = std::max(need, doff[group_end(g0)] - doff[g0]);
    FCX_TRY(V.buf.reserve(need + 64, "verify buffer"));
    V.groups = ngroups;
    const uint32_t cpb = (B + kVChunk - 1) / kVChunk;
    for (uint32_t g0 = 0; g0 < nblocks;) {
        const uint32_t g1 = group_end(g0), nrec = g1 - g0;
        const uint64_t gbytes = doff[g1] - doff[g0];
        uint64_t got = 0;
        mark(1);
        // (an index entry can only lie inside the run: the index was built from it just now)
        if (kind == '7')
            FCX_TRY(fcx_decompress_shard(c, d_rec + roff[g0], rec_len - roff[g0], nrec, V.buf, gbytes, &got, st));
        else
            FCX_TRY(lz78_decompress_shard_at(c, d_rec + roff[g0], rec_len - roff[g0], nrec, V.buf, gbytes, &got, st,
                                             rec_base + g0));
        if (got != gbytes)
            return fail(FCX_ERR_INTERNAL, "fcx_verify_shard: the decode of a group disagrees with the index");
        mark(2);
        if (gbytes && n)
            hipLaunchKernelGGL(k_vcompare, dim3(nrec * cpb), dim3(kVThreads), 0, st, V.buf, doff[g0], R.dec_off, g0, cpb,
                               d_orig, n, B, V.first_diff);
        mark(3);
        FCX_HIP(hipGetLastError());
        if (prof) FCX_TRY(T->add(1, 3));
        g0 = g1;
    }
    mark(3);
    hipLaunchKernelGGL(k_vsummary, dim3(1), dim3(1024), 0, st, nblocks, R.dec_off, n, B, V.first_diff, d_blocks, V.words);
    mark(4);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(V.host_words, V.words, 8 * kVwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < FCX_VERIFY_STATS; i++) stats[i] = V.host_words[i];
    c->times.reset();
    if (prof) {   // the call's own table replaces the last inner decode's
        FCX_TRY(T->add(3, 4));
        for (int i = 0; i < kVStages; i++) c->times.ms[i] = T->ms[i];
        c->times.publish(kVStageNames, kVStages);
    }
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_verify_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                     const uint8_t *d_orig, uint64_t n, uint32_t block_bytes, uint32_t *d_blocks, uint64_t *stats,
                     void *stream) {
    if (!c || !stats) return fail(FCX_ERR_ARG, "fcx_verify_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_verify_shard: kind must be '7' or '8'");
    if (block_bytes == 0 || block_bytes > FCX_MAX_BLOCK_BYTES)
        return fail(FCX_ERR_ARG, "fcx_verify_shard: block_bytes outside [1, FCX_MAX_BLOCK_BYTES]");
    if ((n + block_bytes - 1) / block_bytes != nblocks)
        return fail(FCX_ERR_ARG, "fcx_verify_shard: nblocks is not ceil(n / block_bytes)");
    if (nblocks && (!d_rec || !d_orig)) return fail(FCX_ERR_ARG, "fcx_verify_shard: NULL argument");
    return verify_run(c, kind, d_rec, rec_len, nblocks, d_orig, n, block_bytes, d_blocks, stats, (hipStream_t)stream, 0);
}

int fcx_dctx_set_verify_group(fcx_dctx *c, uint64_t bytes) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    c->vf.group_bytes = bytes;
    return FCX_OK;
}

int fcx_dctx_verify_groups(fcx_dctx *c) { return c ? (int)c->vf.groups : -1; }

}  // extern "C"
