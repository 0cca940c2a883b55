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
//
// The host half of such a run is the run core's (fcx_run.hip).
#include <hip/hip_runtime.h>

#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_device.h"   // wave_max_dpp
#include "fcx_ld16.h"     // ld16_bounded, block_len, publish_verdict

namespace fcx {

constexpr uint32_t kVThreads = 256;
constexpr uint32_t kVChunk = 16384;                       // bytes of a block one workgroup compares
constexpr uint32_t kVSteps = kVChunk / (16 * kVThreads);  // 16-byte pieces per lane

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
// side (the original ends at d_orig + n, the decoded bytes at the group's): ld16_bounded.
__global__ __launch_bounds__(kVThreads) void k_vcompare(const uint8_t *__restrict__ dec, uint64_t dec_base,
                                                        const uint64_t *__restrict__ dec_off, uint32_t k0, uint32_t cpb,
                                                        const uint8_t *__restrict__ orig, uint64_t n, uint32_t B,
                                                        uint32_t *__restrict__ first_diff) {
    const uint32_t k = k0 + blockIdx.x / cpb, c = blockIdx.x % cpb;
    const uint64_t o0 = (uint64_t)k * B, d0 = dec_off[k];
    const uint32_t blen = block_len(k, n, B);
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
        uint32_t f = 16;
        if (i + 16 <= m) {
            f = first_diff16(ld16_bounded(pa, i, sa, blen), ld16_bounded(pb, i, sb, dlen));
        } else {   // the last piece of the common prefix, cut short
            for (uint32_t j = m - i; j-- > 0;)
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
        const uint32_t blen = block_len(k, n, B);
        const uint32_t dlen = (uint32_t)(dec_off[k + 1] - dec_off[k]);
        uint32_t fd = first_diff[k];
        if (fd == FCX_VERIFY_SAME && dlen != blen) fd = min(dlen, blen);
        if ((uint64_t)k * B >= n) fd = 0;
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
    publish_verdict(differ, first, sized, bytes, nblocks, dec_off, words);
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
    RunTimes T(c, kVStages, st);
    RunIndex ix;
    FCX_TRY(V.first_diff.reserve(4ull * nblocks, "first differences"));
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    FCX_HIP(hipMemsetAsync(V.first_diff, 0xFF, 4ull * nblocks, st));
    FCX_HIP(hipMemsetAsync(V.words, 0, 8 * kVwWords, st));
    FCX_HIP(hipMemsetAsync(V.words + kVwFirst, 0xFF, 8, st));
    FCX_HIP(hipStreamSynchronize(st));
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups));
    const uint32_t cpb = (B + kVChunk - 1) / kVChunk;
    for (const RunGroup &g : groups) {
        const uint32_t nrec = g.g1 - g.g0;
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, nrec, V.buf, g.gbytes, st, rec_base, "fcx_verify_shard"));
        T.mark(2);
        if (g.gbytes && n)
            hipLaunchKernelGGL(k_vcompare, dim3(nrec * cpb), dim3(kVThreads), 0, st, V.buf, ix.doff[g.g0], R.dec_off, g.g0, cpb,
                               d_orig, n, B, V.first_diff);
        T.mark(3);
        FCX_HIP(hipGetLastError());
        FCX_TRY(T.add(1, 3));
    }
    T.mark(3);
    hipLaunchKernelGGL(k_vsummary, dim3(1), dim3(1024), 0, st, nblocks, R.dec_off, n, B, V.first_diff, d_blocks, V.words);
    T.mark(4);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(V.host_words, V.words, 8 * kVwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < FCX_VERIFY_STATS; i++) stats[i] = V.host_words[i];
    FCX_TRY(T.add(3, 4));
    T.publish(c, kVStageNames, kVStages);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_verify_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                     const uint8_t *d_orig, uint64_t n, uint32_t block_bytes, uint32_t *d_blocks, uint64_t *stats,
                     void *stream) {
    if (!stats) return fail(FCX_ERR_ARG, "fcx_verify_shard: NULL argument");
    FCX_TRY(run_args("fcx_verify_shard", c, kind, d_rec, nblocks, n, block_bytes));
    if (nblocks && !d_orig) return fail(FCX_ERR_ARG, "fcx_verify_shard: NULL argument");
    return verify_run(c, kind, d_rec, rec_len, nblocks, d_orig, n, block_bytes, d_blocks, stats, (hipStream_t)stream, 0);
}

}  // extern "C"
