// fcx_cut.hip — cut on a device-resident run (gfx950): which bytes of which lines belong to the selected fields or
// byte columns?  fcx_cut_buffer, fcx_cut_shard, fcx_cut_ranges_shard and fcx_cut_ranges_host of include/fcx.h; the
// LIST compiler and the rule on the host: fcx_cut.h.  DESIGN.md §9m.
//
//   the run      on the run core: index, then per record group the decode into the verification's
//                bounded buffer and the kernels below.  A byte's column is the number of ticks between its line's
//                start and itself, so what a group needs of the one before it is a number: the open line's ticks,
//                saturated at kCutSat.  It stays on the device (kKwTicks), as do the output bytes so far.
//   tiles        4096 bytes, 256 lanes x 16.  A stretch of bytes is summarised as (holds d, ticks behind its last d,
//                or all its ticks when it holds none), packed into a word; a o b = b.has ? b : (a.has, sat(a.ticks +
//                b.ticks)) is associative because the bound is fixed.
//   k_ksum       a workgroup per tile: the lanes' summaries from two 16-bit masks, folded by shuffles and through LDS.
//   k_kentry     one workgroup of 1024 threads over contiguous stretches of tiles: the ticks at every tile's entry,
//                scanned from the carried word, and the carry for the next range.
//   k_kmark      per tile: the same fold as an exclusive scan over the lanes, then each lane walks its 16 bytes
//                against the selection table in LDS: 16 keep bits per lane, the tile's kept bytes, the counters.
//   k_kbase      one workgroup: the exclusive scan of the kept counts on top of the call's output bytes so far.
//   k_kgather    per tile: bytes and keep bits again, compacted through LDS at the destination's alignment, stored
//                as a head of bytes, a body of aligned 16-byte vector stores and a tail of bytes, clipped to cap.
//                The size query skips it.
// No workgroup waits for another; every 16-byte read goes through ld16_bounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_cut.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"

namespace fcx {

constexpr uint32_t kKThreads = 256;
constexpr uint32_t kKWaves = kKThreads / 64;
constexpr uint32_t kKTile = 4096;                  // 16 bytes per lane
constexpr uint32_t kKHas = 0x80000000u;            // a summary word: the stretch holds a delimiter
constexpr uint32_t kKMaxGrid = 2048;               // workgroups of k_kmark at most
constexpr uint32_t kKBaseThreads = 1024;
constexpr uint64_t kKMaxGroup = 0xFFFF0000ull;     // bytes of a group at most (u32 counts)
constexpr uint64_t kKPiece = 1ull << 30;           // a plain buffer is cut in pieces of this many bytes

// a o b over summary words
__device__ inline uint32_t kop(uint32_t a, uint32_t b) {
    if (b & kKHas) return b;
    return (a & kKHas) | min((a & ~kKHas) + b, kCutSat);
}

// inclusive scan of the summaries over the wave's lanes
__device__ inline uint32_t wave_kscan(uint32_t s, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(s, o, 64);
        if (lane >= (uint32_t)o) s = kop(u, s);
    }
    return s;
}

// bit 7 of every byte of x that is zero, and of no other (the carry-free form)
__device__ inline uint32_t kzero(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }

// the bytes of w equal to the byte replicated in rep, as bits 0 .. 15 in byte order
__device__ inline uint32_t eq_bits(const uint32_t w[4], uint32_t rep) {
    uint32_t b = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) b |= ((((kzero(w[q] ^ rep) >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * q);
    return b;
}

// The up to 16 bytes at i (a multiple of 16) of [src, src + len) as four dwords, zeros from len on; sh = address of
// src & 15.  Returns the bytes inside the range (0 .. 16).  Nothing outside the range is read.
__device__ inline uint32_t lane_bytes(const uint8_t *__restrict__ src, uint64_t i, uint32_t sh, uint64_t len, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (i >= len) return 0;
    if (i + 16 <= len) {
        const uint4 v = ld16_bounded(src, i, sh, len);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return 16;
    }
    const uint32_t nb = (uint32_t)(len - i);   // the range's last bytes
#pragma unroll
    for (uint32_t q = 0; q < 16; q++)
        if (q < nb) w[q >> 2] |= (uint32_t)src[i + q] << (8 * (q & 3));
    return nb;
}

// the lane's delimiter bits and tick bits (fields: the separators; bytes: every byte that is no delimiter)
template <bool FIELDS>
__device__ inline void lane_masks(const uint32_t w[4], uint32_t nb, uint32_t delim, uint32_t sep, uint32_t &dmask, uint32_t &tmask) {
    const uint32_t in = nb >= 16 ? 0xFFFFu : (1u << nb) - 1;
    dmask = eq_bits(w, delim * 0x01010101u) & in;
    tmask = FIELDS ? eq_bits(w, sep * 0x01010101u) & in : in & ~dmask;
}

__device__ inline uint32_t lane_summary(uint32_t dmask, uint32_t tmask) {
    if (!dmask) return (uint32_t)__popc(tmask);
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(dmask);
    return kKHas | (uint32_t)__popc(tmask >> (hb + 1));
}

// tile_sum[k] = the summary of tile k of [src, src + len)
template <bool FIELDS>
__global__ __launch_bounds__(kKThreads) void k_ksum(const uint8_t *__restrict__ src, uint64_t len, uint32_t delim, uint32_t sep,
                                                   uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t sW[kKWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
    uint32_t w[4], dmask, tmask;
    const uint32_t nb = lane_bytes(src, (uint64_t)blockIdx.x * kKTile + 16ull * t, sh, len, w);
    lane_masks<FIELDS>(w, nb, delim, sep, dmask, tmask);
    const uint32_t inc = wave_kscan(lane_summary(dmask, tmask), lane);
    if (lane == 63) sW[wv] = inc;
    __syncthreads();
    if (t == 0) {
        uint32_t s = sW[0];
        for (uint32_t q = 1; q < kKWaves; q++) s = kop(s, sW[q]);
        tile_sum[blockIdx.x] = s;
    }
}

// One workgroup: tile_entry[k] = the open line's ticks at the first byte of tile k, from words[kKwTicks] and the
// summaries of the tiles before k; words[kKwTicks] = the same behind the last tile.
__global__ __launch_bounds__(kKBaseThreads) void k_kentry(const uint32_t *__restrict__ tile_sum, uint32_t ntiles,
                                                          uint32_t *__restrict__ tile_entry, uint64_t *__restrict__ words) {
    __shared__ uint32_t sW[kKBaseThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6, per = (ntiles + kKBaseThreads - 1) / kKBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    const uint32_t carry = (uint32_t)words[kKwTicks];
    uint32_t s = 0;
    for (uint32_t k = k0; k < k1; k++) s = kop(s, tile_sum[k]);
    const uint32_t inc = wave_kscan(s, lane);
    if (lane == 63) sW[wv] = inc;
    __syncthreads();
    uint32_t cur = carry, all = carry;
    for (uint32_t q = 0; q < kKBaseThreads / 64; q++) {
        if (q < wv) cur = kop(cur, sW[q]);
        all = kop(all, sW[q]);
    }
    const uint32_t up = __shfl_up(inc, 1, 64);
    if (lane) cur = kop(cur, up);
    for (uint32_t k = k0; k < k1; k++) {
        tile_entry[k] = cur & ~kKHas;
        cur = kop(cur, tile_sum[k]);
    }
    if (t == 0) words[kKwTicks] = all & ~kKHas;
}

// keep_bits[256 k + lane] = the keep bits of the lane's 16 bytes of tile k, tile_count[k] = the tile's kept bytes;
// words: the counters advance.  sel: the cut's table (kCutSelWords words), mn its smallest selected column.
template <bool FIELDS>
__global__ __launch_bounds__(kKThreads) void k_kmark(const uint8_t *__restrict__ src, uint64_t len, uint32_t delim, uint32_t sep, uint32_t mn,
                                                    const uint32_t *__restrict__ sel, const uint32_t *__restrict__ tile_entry,
                                                    uint32_t ntiles, uint16_t *__restrict__ keep_bits, uint32_t *__restrict__ tile_count,
                                                    uint64_t *__restrict__ words) {
    __shared__ uint32_t sSel[kCutSelWords];
    __shared__ uint32_t sW[kKWaves];
    __shared__ uint64_t sC[kKWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
    if (t < kCutSelWords) sSel[t] = sel[t];
    uint64_t judged = 0, nd_all = 0, ns_all = 0, nk_all = 0;   // (thread 0's)
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint32_t w[4], dmask, tmask;
        const uint32_t nb = lane_bytes(src, (uint64_t)tile * kKTile + 16ull * t, sh, len, w);
        lane_masks<FIELDS>(w, nb, delim, sep, dmask, tmask);
        const uint32_t inc = wave_kscan(lane_summary(dmask, tmask), lane);
        if (lane == 63) sW[wv] = inc;
        __syncthreads();   // (the first time round: sSel too)
        uint32_t cur = tile_entry[tile];
        for (uint32_t q = 0; q < kKWaves; q++)
            if (q < wv) cur = kop(cur, sW[q]);
        const uint32_t up = __shfl_up(inc, 1, 64);
        if (lane) cur = kop(cur, up);
        uint32_t ticks = cur & ~kKHas, keep = 0, nk = 0;
#pragma unroll
        for (uint32_t q = 0; q < 16; q++) {
            const uint32_t bit = 1u << q;
            if (dmask & bit) {
                keep |= bit;
                ticks = 0;
            } else if (FIELDS && (tmask & bit)) {   // a separator opens column ticks + 2
                const uint32_t k = ticks + 2, i = min(k, kCutSat);
                if (((sSel[i >> 5] >> (i & 31)) & 1u) && k > mn) {
                    keep |= bit;
                    nk++;
                }
                ticks = min(ticks + 1, kCutSat);
            } else if (q < nb) {
                const uint32_t i = min(ticks + 1, kCutSat);
                if ((sSel[i >> 5] >> (i & 31)) & 1u) keep |= bit;
                if (!FIELDS) ticks = min(ticks + 1, kCutSat);
            }
        }
        keep_bits[(uint64_t)tile * kKThreads + t] = (uint16_t)keep;
        // kept bytes, delimiters, separators and kept separators: 16 bits each (<= 4096 per tile)
        uint64_t pk = (uint64_t)__popc(keep) | (uint64_t)__popc(dmask) << 16 | (uint64_t)(FIELDS ? __popc(tmask) : 0) << 32 | (uint64_t)nk << 48;
        pk = wave_sum_u64(pk);
        if (lane == 0) sC[wv] = pk;
        __syncthreads();
        if (t == 0) {
            uint64_t c = 0;
            for (uint32_t q = 0; q < kKWaves; q++) c += sC[q];
            tile_count[tile] = (uint32_t)(c & 0xFFFF);
            judged += min((uint64_t)kKTile, len - (uint64_t)tile * kKTile);
            nd_all += (c >> 16) & 0xFFFF;
            ns_all += (c >> 32) & 0xFFFF;
            nk_all += c >> 48;
        }
        __syncthreads();   // (sW and sC are written again)
    }
    if (t == 0) {
        unsigned long long *wd = (unsigned long long *)words;
        if (judged) atomicAdd(wd + kKwJudged, (unsigned long long)judged);
        if (nd_all) atomicAdd(wd + kKwDelims, (unsigned long long)nd_all);
        if (ns_all) atomicAdd(wd + kKwSeps, (unsigned long long)ns_all);
        if (nk_all) atomicAdd(wd + kKwSepsKept, (unsigned long long)nk_all);
    }
}

// One workgroup: tile_base[k] = kept bytes of the range's tiles before k; words: kKwGroupBase = the call's output
// bytes before this range, kKwOut advanced by the range's.
__global__ __launch_bounds__(kKBaseThreads) void k_kbase(const uint32_t *__restrict__ tile_count, uint32_t ntiles,
                                                         uint32_t *__restrict__ tile_base, uint64_t *__restrict__ words) {
    __shared__ uint32_t sh[kKBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (ntiles + kKBaseThreads - 1) / kKBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    uint32_t s = 0, tot;
    for (uint32_t k = k0; k < k1; k++) s += tile_count[k];
    uint32_t run = block_xscan(s, sh, &tot);
    for (uint32_t k = k0; k < k1; k++) {
        tile_base[k] = run;
        run += tile_count[k];
    }
    if (t == 0) {
        const uint64_t before = words[kKwOut];
        words[kKwGroupBase] = before;
        words[kKwOut] = before + tot;
    }
}

// The kept bytes of tile k to d_out[o, o + count) for o = kKwGroupBase + tile_base[k], as far as they lie in front of
// cap.  They are compacted into LDS from byte (address of d_out + o) & 15 on, so that a 16-byte piece of LDS is an
// aligned 16-byte piece of the output: whole pieces go by vector stores, the head and the tail byte by byte.
__global__ __launch_bounds__(kKThreads) void k_kgather(const uint8_t *__restrict__ src, uint64_t len, const uint16_t *__restrict__ keep_bits,
                                                      const uint32_t *__restrict__ tile_count, const uint32_t *__restrict__ tile_base,
                                                      const uint64_t *__restrict__ words, uint8_t *__restrict__ d_out, uint64_t cap) {
    __shared__ alignas(16) uint8_t sB[kKTile + 16];
    __shared__ uint32_t sS[kKWaves];
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    const uint32_t cnt = tile_count[tile];
    const uint64_t o = words[kKwGroupBase] + tile_base[tile];
    if (cnt == 0 || o >= cap) return;   // (the whole workgroup)
    const uint32_t n = (uint32_t)min((uint64_t)cnt, cap - o);
    const uint32_t a = (uint32_t)((uintptr_t)(d_out + o) & 15);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
    uint32_t w[4];
    const uint32_t nb = lane_bytes(src, (uint64_t)tile * kKTile + 16ull * t, sh, len, w);
    const uint32_t keep = nb ? keep_bits[(uint64_t)tile * kKThreads + t] : 0u;
    uint32_t tot;
    uint32_t pos = a + block_xscan((uint32_t)__popc(keep), sS, &tot);   // pos + popc(keep) <= a + cnt <= 15 + 4096
#pragma unroll
    for (uint32_t q = 0; q < 16; q++)
        if (keep & (1u << q)) sB[pos++] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
    __syncthreads();
    uint8_t *dst = d_out + o - a;   // 16-byte aligned; bytes [a, e) of it are this tile's
    const uint32_t e = a + n, j0 = a ? 1 : 0, j1 = e / 16;
    if (a && t >= a && t < min(16u, e)) dst[t] = sB[t];
    for (uint32_t j = j0 + t; j < j1; j += kKThreads) ((uint4 *)dst)[j] = ((const uint4 *)sB)[j];
    const uint32_t tail = 16 * max(j0, j1);
    if (tail + t < e && t < 16) dst[tail + t] = sB[tail + t];
}

namespace {
const char *kKStageNames[] = {"index", "decode", "cut", "summary"};
constexpr int kKStages = 4;

int ready(fcx_dctx *c) {
    CutScratch &S = c->ct;
    if (!S.host_words) {
        FCX_TRY(S.words.reserve(8 * kKwWords, "cut words"));
        FCX_TRY(S.sel.reserve(4 * kCutSelWords, "cut table"));
        FCX_HIP(S.host_words.alloc(8 * kKwWords));
    }
    for (uint64_t &v : S.stats) v = 0;
    S.scratch_bytes = 0;
    return FCX_OK;
}

void zero_out(fcx_dctx *c, uint64_t *out_len, uint64_t *stats) {
    *out_len = 0;
    for (uint64_t &v : c->ct.stats) v = 0;
    c->ct.scratch_bytes = 0;
    for (int i = 0; i < FCX_CUT_STATS && stats; i++) stats[i] = 0;
}

// room for the tiles of a range of `most` bytes
int tile_room(CutScratch &S, uint64_t most) {
    const uint64_t tiles = (most + kKTile - 1) / kKTile;
    FCX_TRY(S.keep_bits.reserve(2ull * kKThreads * tiles, "cut keep bits"));
    FCX_TRY(S.tile_sum.reserve(4 * tiles, "cut tile words"));
    FCX_TRY(S.tile_entry.reserve(4 * tiles, "cut tile words"));
    FCX_TRY(S.tile_count.reserve(4 * tiles, "cut tile words"));
    FCX_TRY(S.tile_base.reserve(4 * tiles, "cut tile words"));
    S.scratch_bytes += (2ull * kKThreads + 16) * tiles;
    return FCX_OK;
}

// a call starts: the words zeroed and the cut's table on its way, on st (the cut outlives the call's synchronisation)
int begin(fcx_dctx *c, const fcx_cut *cut, hipStream_t st) {
    CutScratch &S = c->ct;
    FCX_HIP(hipMemsetAsync(S.words, 0, 8 * kKwWords, st));
    FCX_HIP(hipMemcpyAsync(S.sel, cut->sel, 4 * kCutSelWords, hipMemcpyHostToDevice, st));
    return FCX_OK;
}

// the len bytes at src (0 < len <= kKMaxGroup) continue the call's text
template <bool FIELDS>
void launch_range(CutScratch &S, const fcx_cut *cut, const uint8_t *src, uint64_t len, uint8_t *d_out, uint64_t cap, hipStream_t st) {
    const uint32_t ntiles = (uint32_t)((len + kKTile - 1) / kKTile);
    const uint32_t delim = cut->delim, sep = cut->sep;
    hipLaunchKernelGGL(k_ksum<FIELDS>, dim3(ntiles), dim3(kKThreads), 0, st, src, len, delim, sep, (uint32_t *)S.tile_sum);
    hipLaunchKernelGGL(k_kentry, dim3(1), dim3(kKBaseThreads), 0, st, (const uint32_t *)S.tile_sum, ntiles, (uint32_t *)S.tile_entry,
                       (uint64_t *)S.words);
    hipLaunchKernelGGL(k_kmark<FIELDS>, dim3(std::min(ntiles, kKMaxGrid)), dim3(kKThreads), 0, st, src, len, delim, sep, cut->mn,
                       (const uint32_t *)S.sel, (const uint32_t *)S.tile_entry, ntiles, (uint16_t *)S.keep_bits, (uint32_t *)S.tile_count,
                       (uint64_t *)S.words);
    hipLaunchKernelGGL(k_kbase, dim3(1), dim3(kKBaseThreads), 0, st, (const uint32_t *)S.tile_count, ntiles, (uint32_t *)S.tile_base,
                       (uint64_t *)S.words);
    if (cap)
        hipLaunchKernelGGL(k_kgather, dim3(ntiles), dim3(kKThreads), 0, st, src, len, (const uint16_t *)S.keep_bits,
                           (const uint32_t *)S.tile_count, (const uint32_t *)S.tile_base, (const uint64_t *)S.words, d_out, cap);
}

void cut_range(CutScratch &S, const fcx_cut *cut, const uint8_t *src, uint64_t len, uint8_t *d_out, uint64_t cap, hipStream_t st) {
    if (len == 0) return;
    if (cut->mode == FCX_CUT_FIELDS) launch_range<true>(S, cut, src, len, d_out, cap, st);
    else launch_range<false>(S, cut, src, len, d_out, cap, st);
}

// the words on their way to the host ...
int fetch(fcx_dctx *c, hipStream_t st) {
    CutScratch &S = c->ct;
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(S.host_words, S.words, 8 * kKwWords, hipMemcpyDeviceToHost, st));
    return FCX_OK;
}

// ... and, once st is synchronised, into the stats
int finish(fcx_dctx *c, uint64_t *out_len, uint64_t *stats, hipStream_t st) {
    CutScratch &S = c->ct;
    FCX_HIP(hipStreamSynchronize(st));
    const uint64_t *hw = S.host_words;
    S.stats[0] = hw[kKwOut];
    S.stats[1] = hw[kKwJudged];
    S.stats[2] = hw[kKwDelims];
    S.stats[3] = hw[kKwSeps];
    S.stats[4] = hw[kKwSepsKept];
    *out_len = hw[kKwOut];
    for (int i = 0; i < FCX_CUT_STATS && stats; i++) stats[i] = S.stats[i];
    return FCX_OK;
}

// fcx_cut_buffer behind its argument checks; `extra`: scratch bytes a caller reserved in front of it
int cut_buffer(fcx_dctx *c, const uint8_t *d_in, uint64_t n, const fcx_cut *cut, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
               uint64_t *stats, hipStream_t st, uint64_t extra) {
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    CutScratch &S = c->ct;
    S.scratch_bytes = extra;
    FCX_TRY(tile_room(S, std::min(n, kKPiece)));
    FCX_TRY(begin(c, cut, st));
    for (uint64_t at = 0; at < n; at += kKPiece) {
        cut_range(S, cut, d_in + at, std::min(kKPiece, n - at), d_out, cap, st);
        S.stats[5]++;
    }
    FCX_TRY(fetch(c, st));
    return finish(c, out_len, stats, st);
}
}  // namespace

int cut_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_cut *cut, uint8_t *d_out,
            uint64_t cap, uint64_t *out_len, uint64_t *stats, hipStream_t st, uint64_t rec_base, bool cont) {
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    CutScratch &S = c->ct;
    VerifyScratch &V = c->vf;
    RunTimes T(c, kKStages, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    if (cont) FCX_HIP(hipMemsetAsync((uint64_t *)S.words + kKwOut, 0, 8, st));   // (this run's output starts at d_out again)
    else FCX_TRY(begin(c, cut, st));
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host)
    FCX_TRY(T.add(0, 1));
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most > kKMaxGroup) return fail(FCX_ERR_ARG, "fcx_cut_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    FCX_TRY(tile_room(S, most));
    for (const RunGroup &g : groups) {
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, V.buf, g.gbytes, st, rec_base, "fcx_cut_shard"));
        T.mark(2);
        cut_range(S, cut, V.buf, g.gbytes, d_out, cap, st);
        T.mark(3);
        FCX_HIP(hipGetLastError());
        FCX_TRY(T.add(1, 3));
        S.stats[5]++;
    }
    T.mark(3);
    FCX_TRY(fetch(c, st));
    T.mark(4);
    FCX_TRY(finish(c, out_len, stats, st));
    FCX_TRY(T.add(3, 4));
    T.publish(c, kKStageNames, kKStages);
    return FCX_OK;
}

int cut_ranges_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint64_t *d_rec_off,
                   const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end, uint64_t nranges, const fcx_cut *cut,
                   uint8_t *d_out, uint64_t cap, uint64_t *out_len, uint64_t *stats, hipStream_t st) {
    zero_out(c, out_len, stats);
    if (nranges == 0) return FCX_OK;
    // the ranges' sum first (the multi-range decode's size query: it checks the ranges and, without an index, leaves
    // the run's in the range API's scratch), then their bytes, then the buffer cut
    uint64_t sum = 0, got = 0;
    const int rc = ranges_run(c, kind, d_rec, rec_len, nblocks, d_rec_off, d_dec_off, d_start, d_end, nranges, nullptr, 0, &sum, st);
    if (rc != FCX_OK && !(rc == FCX_ERR_CAPACITY && sum > 0)) return rc;
    if (sum == 0) return FCX_OK;
    CutScratch &S = c->ct;
    FCX_TRY(S.gathered.reserve(sum, "cut ranges buffer"));
    const uint64_t *ro = d_rec_off ? d_rec_off : (const uint64_t *)c->rg.rec_off, *dof = d_rec_off ? d_dec_off : (const uint64_t *)c->rg.dec_off;
    FCX_TRY(ranges_run(c, kind, d_rec, rec_len, nblocks, ro, dof, d_start, d_end, nranges, S.gathered, sum, &got, st));
    if (got != sum) return fail(FCX_ERR_INTERNAL, "fcx_cut_ranges_shard: the ranges' bytes disagree with their sum");
    c->times.reset();   // (not the inner decode's table)
    return cut_buffer(c, S.gathered, sum, cut, d_out, cap, out_len, stats, st, sum);
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_cut_create(fcx_cut **cut, const char *list, uint32_t len, uint32_t mode, uint8_t sep, uint8_t delim, uint32_t flags) {
    if (!cut) return fail(FCX_ERR_ARG, "fcx_cut_create: NULL argument");
    *cut = nullptr;
    std::unique_ptr<fcx_cut> c(new fcx_cut());
    const std::string why = cut_compile(c.get(), list, len, mode, sep, delim, flags);
    if (!why.empty()) return fail(FCX_ERR_ARG, "fcx_cut_create: " + why);
    *cut = c.release();
    return FCX_OK;
}

void fcx_cut_destroy(fcx_cut *cut) { delete cut; }

int fcx_cut_info(const fcx_cut *cut, uint32_t *mode, uint8_t *sep, uint8_t *delim, uint32_t *flags, uint32_t *mn, uint32_t *open_end) {
    if (!cut) return fail(FCX_ERR_ARG, "fcx_cut_info: NULL argument");
    if (mode) *mode = cut->mode;
    if (sep) *sep = cut->sep;
    if (delim) *delim = cut->delim;
    if (flags) *flags = cut->flags;
    if (mn) *mn = cut->mn;
    if (open_end) *open_end = cut->open_end;
    return FCX_OK;
}

int fcx_cut_buffer(fcx_dctx *c, const uint8_t *d_in, uint64_t n, const fcx_cut *cut, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                   uint64_t *stats, void *stream) {
    if (!c || !cut || !out_len || (n && !d_in) || (cap && !d_out)) return fail(FCX_ERR_ARG, "fcx_cut_buffer: NULL argument");
    zero_out(c, out_len, stats);
    if (n == 0) return FCX_OK;
    c->times.reset();
    return cut_buffer(c, d_in, n, cut, d_out, cap, out_len, stats, (hipStream_t)stream, 0);
}

int fcx_cut_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_cut *cut, uint8_t *d_out,
                  uint64_t cap, uint64_t *out_len, uint64_t *stats, void *stream) {
    if (!c || !cut || !out_len || (nblocks && !d_rec) || (cap && !d_out)) return fail(FCX_ERR_ARG, "fcx_cut_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_cut_shard: kind must be '7' or '8'");
    zero_out(c, out_len, stats);
    if (nblocks == 0) return FCX_OK;
    return cut_run(c, kind, d_rec, rec_len, nblocks, cut, d_out, cap, out_len, stats, (hipStream_t)stream, 0, false);
}

int fcx_cut_ranges_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint64_t *d_rec_off,
                         const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end, uint64_t nranges, const fcx_cut *cut,
                         uint8_t *d_out, uint64_t cap, uint64_t *out_len, uint64_t *stats, void *stream) {
    if (!c || !cut || !out_len || (nblocks && !d_rec) || (nranges && (!d_start || !d_end)) || (cap && !d_out))
        return fail(FCX_ERR_ARG, "fcx_cut_ranges_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_cut_ranges_shard: kind must be '7' or '8'");
    if (!d_rec_off != !d_dec_off) return fail(FCX_ERR_ARG, "fcx_cut_ranges_shard: half an index (one pointer NULL)");
    return cut_ranges_run(c, kind, d_rec, rec_len, nblocks, d_rec_off, d_dec_off, d_start, d_end, nranges, cut, d_out, cap, out_len, stats,
                          (hipStream_t)stream);
}

int fcx_dctx_cut_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_cut_stats: bad argument");
    for (int i = 0; i < n && i < FCX_CUT_STATS; i++) out[i] = c->ct.stats[i];
    return FCX_OK;
}

int fcx_dctx_cut_scratch(fcx_dctx *c, uint64_t *bytes) {
    if (!c || !bytes) return fail(FCX_ERR_ARG, "fcx_dctx_cut_scratch: NULL argument");
    *bytes = c->ct.scratch_bytes;
    return FCX_OK;
}

}  // extern "C"
