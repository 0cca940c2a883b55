// fcx_find.hip — search of a device-resident run (gfx950): where do the bytes of a pattern occur in what the
// records decode to?  fcx_find_shard of include/fcx.h (its stream and host forms: fcx_stream.hip).
// DESIGN.md §9g.
//
//   the run      on the run core: index, then per record group the decode into the
//                verification's bounded buffer at buf + kFCarry; the bytes in front hold the carry, the last
//                min(m - 1, bytes seen) decoded bytes before the group, so [carry | group] is one byte
//                range and a group's scan judges the start positions p in it with p + m <= group end.
//                What is left over (the last m - 1 positions) is judged with the next group; the carry
//                is kept in a buffer of its own (k_fcarry), so it may span any number of short or empty
//                groups and outlives the buffer's growth between the stream form's calls.
//   k_fscan      workgroup of 256 lanes per tile of 4096 start positions, grid-strided: the tile and m - 1
//                bytes behind it go to LDS by 16-byte pieces through ld16_bounded (nothing outside the
//                range is read), the pattern too.  Lane t reads its 16 bytes with one ds_read_b128
//                (conflict-free: consecutive 16-byte slots) and takes the 4 bytes behind them from lane
//                t + 1's registers: a ds_read_b32 at a 16-byte stride would be 4-way conflicted (8 banks
//                for 32 lanes), so only the last lane of a wave reads them from LDS.  16 positions per
//                lane: the first min(m, 4) bytes as one masked 32-bit compare, the rest of the pattern
//                dword by dword from LDS only where that passes.  16 hit bits per lane to the tile's 512 B
//                of bitmap, the tile's count, and per workgroup one atomic add each of the judged and
//                candidate counts.
//   k_fbase      one workgroup: the exclusive scan of the tile counts, and the call's hits so far.
//   k_fwrite     per tile with hits whose ranks meet the window: rank of each set bit by popcount and
//                prefix, base offset + position as u64 to out[rank - window start].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"

namespace fcx {

constexpr uint32_t kFThreads = 256;
constexpr uint32_t kFPer = 16;                                // start positions per lane
constexpr uint32_t kFTile = kFPer * kFThreads;                // start positions per tile (4096)
constexpr uint32_t kFPieces = (kFTile + kFCarry + 15) / 16;   // 16-byte pieces of a tile and its halo at most
constexpr uint32_t kFLdsBytes = 16 * kFPieces + 16;           // (+ 16: the dword behind the last lane's bytes)
constexpr uint32_t kFMaxGrid = 2048;                          // workgroups of k_fscan / k_fwrite at most
constexpr uint32_t kFBaseThreads = 1024;
constexpr uint32_t kFWindow = 1u << 20;                       // hits per window of the stream form by default
constexpr uint64_t kFMaxRange = 0xFFFF0000ull;                // bytes of [carry | group] at most

// bytes [4, m) of the pattern against the LDS bytes at q + 4 ... (the first 4 passed the filter)
__device__ inline bool find_rest(const uint32_t *sT, const uint32_t *sP, uint32_t q, uint32_t m) {
    const uint32_t w0 = q >> 2, bs = q & 3, nd = (m + 3) >> 2;
    uint32_t lo = sT[w0 + 1];
    for (uint32_t j = 1; j < nd; j++) {
        const uint32_t hi = sT[w0 + j + 1];
        uint32_t d = __builtin_amdgcn_alignbyte(hi, lo, bs) ^ sP[j];
        if (j + 1 == nd && (m & 3)) d &= (1u << (8 * (m & 3))) - 1;
        if (d) return false;
        lo = hi;
    }
    return true;
}

// The start positions [0, njudged) of the byte range [src, src + len), njudged = len - m + 1: bit p & 15 of
// bitmap[p >> 4] says whether src[p, p + m) is the pattern (pat: its bytes, zero-padded to kFCarry);
// positions from njudged on in the last tile get 0.  tile_count[k]: hits of tile k.  words: kFwJudged and
// kFwCand advance.
__global__ __launch_bounds__(kFThreads) void k_fscan(const uint8_t *__restrict__ src, uint64_t len, uint64_t njudged, uint32_t m,
                                                     const uint32_t *__restrict__ pat, uint32_t ntiles,
                                                     uint16_t *__restrict__ bitmap, uint32_t *__restrict__ tile_count,
                                                     uint64_t *__restrict__ words) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kFLdsBytes / 4];
    __shared__ uint32_t sP[kFCarry / 4];
    __shared__ uint32_t sC[kFThreads / 64];
    __shared__ uint64_t sJ[2 * (kFThreads / 64)];
    const uint32_t t = threadIdx.x;
    if (t < kFCarry / 4) sP[t] = pat[t];
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
    const uint32_t pmask = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1, p0 = pat[0] & pmask;
    const uint32_t npieces = (kFTile + m - 1 + 15) / 16;   // (<= kFPieces)
    uint64_t judged = 0, cand = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kFTile;
        __syncthreads();   // the readers of the tile before are done (the first round: sP is there)
        for (uint32_t j = t; j < npieces; j += kFThreads) {
            const uint64_t i = base + 16ull * j;
            uint4 w = make_uint4(0, 0, 0, 0);
            if (i + 16 <= len) {
                w = ld16_bounded(src, i, sh, len);
            } else if (i < len) {   // the range's last bytes
                uint32_t x[4] = {0, 0, 0, 0};
                for (uint32_t q = 0; q < (uint32_t)(len - i); q++) x[q >> 2] |= (uint32_t)src[i + q] << (8 * (q & 3));
                w = make_uint4(x[0], x[1], x[2], x[3]);
            }
            ((uint4 *)sT)[j] = w;
        }
        __syncthreads();
        const uint64_t at = base + kFPer * t;   // this lane's first position
        const uint32_t nj = at >= njudged ? 0u : (uint32_t)min((uint64_t)kFPer, njudged - at);
        const uint4 a = ((const uint4 *)sT)[t];
        uint32_t e = __shfl_down(a.x, 1, 64);
        if ((t & 63) == 63) e = sT[4 * t + 4];
        const uint32_t w[5] = {a.x, a.y, a.z, a.w, e};
        uint32_t c = 0;
#pragma unroll
        for (uint32_t b = 0; b < kFPer; b++) {
            const uint32_t v = __builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3);
            c |= (uint32_t)(((v ^ p0) & pmask) == 0) << b;
        }
        c &= (1u << nj) - 1;
        judged += nj;
        cand += __popc(c);
        uint32_t hits = c;
        if (m > 4) {
            hits = 0;
            while (c) {
                const uint32_t b = (uint32_t)__builtin_ctz(c);
                c &= c - 1;
                if (find_rest(sT, sP, kFPer * t + b, m)) hits |= 1u << b;
            }
        }
        bitmap[(uint64_t)tile * kFThreads + t] = (uint16_t)hits;
        uint32_t n = __popc(hits);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if ((t & 63) == 0) sC[t >> 6] = n;
        __syncthreads();
        if (t == 0) tile_count[tile] = sC[0] + sC[1] + sC[2] + sC[3];
    }
    judged = wave_sum_u64(judged);
    cand = wave_sum_u64(cand);
    if ((t & 63) == 0) {
        sJ[2 * (t >> 6)] = judged;
        sJ[2 * (t >> 6) + 1] = cand;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long *w = (unsigned long long *)words;
        atomicAdd(w + kFwJudged, (unsigned long long)(sJ[0] + sJ[2] + sJ[4] + sJ[6]));
        atomicAdd(w + kFwCand, (unsigned long long)(sJ[1] + sJ[3] + sJ[5] + sJ[7]));
    }
}

// One workgroup: tile_base[k] = hits of the group's tiles before k; words: kFwGroupBase = the call's hits
// before this group, kFwHits advanced by the group's.
__global__ __launch_bounds__(kFBaseThreads) void k_fbase(const uint32_t *__restrict__ tile_count, uint32_t ntiles,
                                                         uint32_t *__restrict__ tile_base, uint64_t *__restrict__ words) {
    __shared__ uint32_t sh[kFBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (ntiles + kFBaseThreads - 1) / kFBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    uint32_t s = 0, tot;
    for (uint32_t k = k0; k < k1; k++) s += tile_count[k];
    uint32_t run = block_xscan(s, sh, &tot);
    for (uint32_t k = k0; k < k1; k++) {
        tile_base[k] = run;
        run += tile_count[k];
    }
    if (t == 0) {
        const uint64_t before = words[kFwHits];
        words[kFwGroupBase] = before;
        words[kFwHits] = before + tot;
    }
}

// The hits of the group whose rank in the call lies in [win0, win0 + winlen): pos_base + position to
// out[rank - win0].  pos_base: the decoded offset of the scanned range's first byte.
__global__ __launch_bounds__(kFThreads) void k_fwrite(const uint16_t *__restrict__ bitmap, const uint32_t *__restrict__ tile_count,
                                                      const uint32_t *__restrict__ tile_base, uint32_t ntiles,
                                                      const uint64_t *__restrict__ words, uint64_t pos_base, uint64_t win0,
                                                      uint64_t winlen, uint64_t *__restrict__ out) {
    __shared__ uint32_t sW[kFThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint64_t group_base = words[kFwGroupBase];
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t cnt = tile_count[tile];
        const uint64_t r0 = group_base + tile_base[tile];
        if (cnt == 0 || r0 + cnt <= win0 || r0 >= win0 + winlen) continue;   // (the whole workgroup)
        uint32_t bits = bitmap[(uint64_t)tile * kFThreads + t];
        const uint32_t n = __popc(bits);
        uint32_t inc = n;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            if (lane >= (uint32_t)o) inc += u;
        }
        __syncthreads();   // sW of the tile before is read
        if (lane == 63) sW[wv] = inc;
        __syncthreads();
        uint64_t rank = r0 + inc - n;
        for (uint32_t q = 0; q < wv; q++) rank += sW[q];
        const uint64_t pos = pos_base + (uint64_t)tile * kFTile + kFPer * t;
        while (bits) {
            const uint32_t b = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1;
            if (rank >= win0 && rank - win0 < winlen) out[rank - win0] = pos + b;
            rank++;
        }
    }
}

// the last `keep` (<= kFCarry) bytes of [src, src + len) to the end of the carry buffer
__global__ __launch_bounds__(kFThreads) void k_fcarry(const uint8_t *__restrict__ src, uint64_t len, uint32_t keep,
                                                      uint8_t *__restrict__ carry) {
    const uint32_t t = threadIdx.x;
    if (t < keep) carry[kFCarry - keep + t] = src[len - keep + t];
}

namespace {
const char *kFStageNames[] = {"index", "decode", "scan", "summary"};
constexpr int kFStages = 4;

int ready(fcx_dctx *c) {
    FindScratch &F = c->fd;
    if (!F.host_words) {
        FCX_TRY(F.words.reserve(8 * kFwWords, "find words"));
        FCX_TRY(F.pat.reserve(kFCarry, "find pattern"));
        FCX_TRY(F.carry.reserve(kFCarry, "find carry"));
        FCX_HIP(F.host_words.alloc(8 * kFwWords));
    }
    for (uint64_t &v : F.stats) v = 0;
    return FCX_OK;
}
}  // namespace

int find_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *pattern, uint32_t m,
             uint64_t base, const FindSink &sink, uint64_t *nhits, uint64_t *decoded, hipStream_t st, uint64_t rec_base) {
    *nhits = 0;
    if (decoded) *decoded = 0;
    if (nblocks == 0) {
        for (uint64_t &v : c->fd.stats) v = 0;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    FindScratch &F = c->fd;
    VerifyScratch &V = c->vf;
    const uint64_t window = F.window ? F.window : kFWindow;
    if (sink.on_hit) FCX_TRY(F.hits.reserve(8 * window, "find hits"));
    RunTimes T(c, kFStages, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    uint8_t padded[kFCarry] = {};
    memcpy(padded, pattern, m);
    FCX_HIP(hipMemcpyAsync(F.pat, padded, kFCarry, hipMemcpyHostToDevice, st));
    FCX_HIP(hipMemsetAsync(F.words, 0, 8 * kFwWords, st));
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host, `padded` may go)
    const std::vector<uint64_t> &doff = ix.doff;
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups, nullptr, kFCarry));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most + kFCarry > kFMaxRange)
        return fail(FCX_ERR_ARG, "fcx_find_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    const uint64_t tiles_most = (most + kFCarry + kFTile - 1) / kFTile;
    FCX_TRY(F.bitmap.reserve(2ull * kFThreads * tiles_most, "find bitmap"));
    FCX_TRY(F.tile_count.reserve(4 * tiles_most, "find tile counts"));
    FCX_TRY(F.tile_base.reserve(4 * tiles_most, "find tile counts"));
    std::vector<uint64_t> host_hits;
    uint8_t *const dec = V.buf + kFCarry;
    for (const RunGroup &g : groups) {
        const uint32_t cl = F.carry_len;
        if (cl) FCX_HIP(hipMemcpyAsync(dec - cl, F.carry + (kFCarry - cl), cl, hipMemcpyDeviceToDevice, st));
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, dec, g.gbytes, st, rec_base, "fcx_find_shard"));
        T.mark(2);
        const uint8_t *src = dec - cl;
        const uint64_t len = cl + g.gbytes, njudged = len >= m ? len - m + 1 : 0;
        const uint32_t ntiles = (uint32_t)((njudged + kFTile - 1) / kFTile);
        const uint32_t grid = std::min(ntiles, kFMaxGrid);
        const uint64_t pos_base = base + doff[g.g0] - cl;
        if (ntiles) {
            hipLaunchKernelGGL(k_fscan, dim3(grid), dim3(kFThreads), 0, st, src, len, njudged, m, (const uint32_t *)F.pat, ntiles,
                               (uint16_t *)F.bitmap, (uint32_t *)F.tile_count, (uint64_t *)F.words);
            hipLaunchKernelGGL(k_fbase, dim3(1), dim3(kFBaseThreads), 0, st, (const uint32_t *)F.tile_count, ntiles,
                               (uint32_t *)F.tile_base, (uint64_t *)F.words);
            if (sink.cap) {
                hipLaunchKernelGGL(k_fwrite, dim3(grid), dim3(kFThreads), 0, st, (const uint16_t *)F.bitmap,
                                   (const uint32_t *)F.tile_count, (const uint32_t *)F.tile_base, ntiles, (const uint64_t *)F.words,
                                   pos_base, 0ull, sink.cap, sink.d_hits);
                F.stats[5]++;
            }
        }
        T.mark(3);
        FCX_HIP(hipGetLastError());
        FCX_TRY(T.add(1, 3));
        // what the next group needs of this one: source and destination are two buffers
        const uint32_t keep = (uint32_t)std::min<uint64_t>(m - 1, len);
        if (keep) hipLaunchKernelGGL(k_fcarry, dim3(1), dim3(kFThreads), 0, st, src, len, keep, (uint8_t *)F.carry);
        F.carry_len = keep;
        F.stats[4] += keep;
        F.stats[3]++;
        if (sink.on_hit && ntiles) {   // the group's hits, window after window of the same bitmap
            FCX_HIP(hipMemcpyAsync(F.host_words, F.words, 8 * kFwWords, hipMemcpyDeviceToHost, st));
            FCX_HIP(hipStreamSynchronize(st));
            const uint64_t before = F.host_words[kFwGroupBase], end = F.host_words[kFwHits];
            for (uint64_t w0 = before; w0 < end; w0 += window) {
                const uint64_t n = std::min(window, end - w0);
                hipLaunchKernelGGL(k_fwrite, dim3(grid), dim3(kFThreads), 0, st, (const uint16_t *)F.bitmap,
                                   (const uint32_t *)F.tile_count, (const uint32_t *)F.tile_base, ntiles, (const uint64_t *)F.words,
                                   pos_base, w0, n, (uint64_t *)F.hits);
                FCX_HIP(hipGetLastError());
                host_hits.resize(n);
                FCX_HIP(hipMemcpyAsync(host_hits.data(), F.hits, 8 * n, hipMemcpyDeviceToHost, st));
                FCX_HIP(hipStreamSynchronize(st));
                for (uint64_t i = 0; i < n; i++) sink.on_hit(sink.user, host_hits[i]);
                F.stats[5]++;
            }
        }
    }
    T.mark(3);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(F.host_words, F.words, 8 * kFwWords, hipMemcpyDeviceToHost, st));
    T.mark(4);
    FCX_HIP(hipStreamSynchronize(st));
    F.stats[0] = F.host_words[kFwJudged];
    F.stats[1] = F.host_words[kFwCand];
    F.stats[2] = F.host_words[kFwHits];
    *nhits = F.host_words[kFwHits];
    if (decoded) *decoded = doff[nblocks];
    FCX_TRY(T.add(3, 4));
    T.publish(c, kFStageNames, kFStages);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_find_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *pattern,
                   uint32_t plen, uint64_t *d_hits, uint64_t cap, uint64_t *nhits, void *stream) {
    if (!c || !pattern || !nhits || (nblocks && !d_rec) || (cap && !d_hits))
        return fail(FCX_ERR_ARG, "fcx_find_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_find_shard: kind must be '7' or '8'");
    if (plen < 1 || plen > FCX_FIND_MAX_PATTERN) return fail(FCX_ERR_ARG, "fcx_find_shard: pattern length outside [1, FCX_FIND_MAX_PATTERN]");
    c->fd.carry_len = 0;
    FindSink sink;
    sink.d_hits = d_hits;
    sink.cap = cap;
    return find_run(c, kind, d_rec, rec_len, nblocks, pattern, plen, 0, sink, nhits, nullptr, (hipStream_t)stream, 0);
}

int fcx_dctx_find_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_find_stats: bad argument");
    for (int i = 0; i < n && i < FCX_FIND_STATS; i++) out[i] = c->fd.stats[i];
    return FCX_OK;
}

int fcx_dctx_set_find_window(fcx_dctx *c, uint32_t hits) {
    if (!c) return fail(FCX_ERR_ARG, "fcx_dctx_set_find_window: NULL ctx");
    c->fd.window = hits;
    return FCX_OK;
}

}  // extern "C"
