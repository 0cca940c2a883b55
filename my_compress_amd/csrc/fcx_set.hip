// fcx_set.hip — pattern sets on a device-resident run (gfx950): at which positions of what the records decode to
// does at least one of up to 64 byte strings occur, with or without ASCII case folding, and which lines hold
// such a position?  fcx_pattern_set_*, fcx_find_set_shard and fcx_grep_set_shard of include/fcx.h (their stream
// and host forms: fcx_stream.hip, fcx_ranges.hip).  DESIGN.md §9j.
//
//   the run      on the run core as the search's and the grep's: index, then per record group the
//                decode to buf + kFCarry with the carry in front.  M = the longest pattern: the carry is the last
//                min(M - 1, bytes seen) bytes, a group that is not the run's last judges the positions p with
//                p + M <= group end against every pattern, and the run's last group (the stream forms: a final
//                pass over the carry alone) judges what is left with pattern k admitted iff p + len_k <= end.
//                The carry is therefore exactly the positions not judged yet, whatever the lengths are.
//   k_sscan      k_fscan's and k_gscan's tile shape (256 lanes, 4096 start positions, the tile and M - 1 bytes
//                behind it in LDS through ld16_bounded).  With the fold flag each 16-byte piece is folded on its
//                way to LDS by word operations, so everything behind the staging compares exactly; the delimiter
//                bits come from the lane's own piece before the fold.  The set's block (fcx_patset.h: lengths,
//                two tables of 256 u64, the pattern bytes) is staged once per workgroup.  A position's candidate
//                mask is T0[b0] & T1[b1], two ds_read_b64 whatever the number of patterns; only positions with a
//                non-zero mask go on, and only the patterns whose bit survived are compared in full, dword by
//                dword against the LDS bytes, after the bound p + len_k <= end.  Per-pattern counts go to 64 LDS
//                counters and from there, once per workgroup and non-zero counter, to the device words.
//   downstream   the search's k_fbase / k_fwrite / k_fcarry and the grep's k_gtiles / k_gmark / k_gbase /
//                k_gwrite / k_gfinish / k_gcarry, unchanged: k_sscan leaves the bitmaps, tile counts and tile
//                summaries in their formats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"
#include "fcx_patset.h"

namespace fcx {

constexpr uint32_t kSThreads = 256;
constexpr uint32_t kSWaves = kSThreads / 64;
constexpr uint32_t kSPer = 16;                                // start positions per lane
constexpr uint32_t kSTile = kSPer * kSThreads;                // start positions per tile (4096)
constexpr uint32_t kSPieces = (kSTile + kFCarry + 15) / 16;   // 16-byte pieces of a tile and its halo at most
constexpr uint32_t kSLdsBytes = 16 * kSPieces + 16;           // (+ 16: the dwords behind the last lane's bytes)
constexpr uint32_t kSMaxGrid = 2048;
constexpr uint32_t kSBaseThreads = 1024;                      // k_fbase, k_gtiles and k_gbase: one workgroup of 1024
constexpr uint32_t kSWindow = 1u << 20;                       // hits or lines per window of the stream forms by default
constexpr uint64_t kSMaxRange = 0xFFFF0000ull;                // bytes of [carry | group] at most
constexpr uint32_t kSNone = 0xFFFFFFFFu;
constexpr uint32_t kSSum = 4, kSCtx = 3;                      // words per tile of the grep's tile_sum / tile_ctx
static_assert((kSTile >> 2) - 1 + kFCarry / 4 + 1 < kSLdsBytes / 4, "set_full reads inside the tile's LDS");

// fold(b) of the four bytes of a dword: bytes in [0x41, 0x5A] get bit 5.  Carry-free: the low seven bits of each
// byte are compared by two additions that cannot leave their byte, bytes >= 0x80 are left alone.
__device__ inline uint32_t fold4(uint32_t x) {
    const uint32_t y = x & 0x7F7F7F7Fu;
    const uint32_t ge_a = y + 0x3F3F3F3Fu;   // bit 7: y >= 0x41
    const uint32_t gt_z = y + 0x25252525u;   // bit 7: y >= 0x5B
    return x | ((ge_a & ~gt_z & ~x & 0x80808080u) >> 2);
}

// bit q of the result: byte q of the dword equals the byte replicated in rep (the carry-free zero-byte form)
__device__ inline uint32_t set_eq_bits4(uint32_t x, uint32_t rep) {
    x ^= rep;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// the m bytes of a pattern (sP: its dwords, zero-padded) against the LDS bytes at q
__device__ inline bool set_full(const uint32_t *sT, const uint32_t *sP, uint32_t q, uint32_t m) {
    const uint32_t w0 = q >> 2, bs = q & 3, nd = (m + 3) >> 2;
    uint32_t lo = sT[w0];
    for (uint32_t j = 0; j < nd; j++) {
        const uint32_t hi = sT[w0 + j + 1];
        uint32_t d = __builtin_amdgcn_alignbyte(hi, lo, bs) ^ sP[j];
        if (j + 1 == nd && (m & 3)) d &= (1u << (8 * (m & 3))) - 1;
        if (d) return false;
        lo = hi;
    }
    return true;
}

// The start positions [0, njudged) of the byte range [src, src + len): bit p & 15 of hit_bits[p >> 4] says whether a
// pattern of the set occurs at p, pattern k being admitted iff p + len_k <= len (njudged = len - M + 1 in a group
// that is not the last admits all of them, len - min_len + 1 at the run's end bounds each).  Positions from njudged
// on get 0.  GREP: delim_bits likewise for src[p] == delim, p < ndelim, over the bytes before the fold, and
// tile_out[4 k ..] = the tile's hits, 1 + its first delimiter, 1 + its last delimiter, 1 + its last hit (k_gscan's
// summary); otherwise tile_out[k] = the tile's hits (k_fscan's count).  block: the set (fcx_patset.h), maxlen its
// longest pattern.  w_judged advances by the positions judged, w_second (may be null) by the hits (GREP) or by the
// positions with a non-zero candidate mask; swords: kSw* advance.
template <bool GREP>
__global__ __launch_bounds__(kSThreads) void k_sscan(const uint8_t *__restrict__ src, uint64_t len, uint64_t njudged, uint64_t ndelim,
                                                     uint32_t maxlen,
                                                     uint32_t fold, uint32_t delim, const uint32_t *__restrict__ block,
                                                     uint32_t ntiles, uint16_t *__restrict__ hit_bits,
                                                     uint16_t *__restrict__ delim_bits, uint32_t *__restrict__ tile_out,
                                                     uint64_t *__restrict__ w_judged, uint64_t *__restrict__ w_second,
                                                     uint64_t *__restrict__ swords) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kSLdsBytes / 4];
    __shared__ __attribute__((aligned(16))) uint32_t sB[kPsWords];
    __shared__ uint32_t sN[FCX_SET_MAX_PATTERNS];
    __shared__ uint32_t sR[4 * kSWaves];
    __shared__ uint64_t sJ[4 * kSWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (uint32_t j = t; j < kPsWords / 4; j += kSThreads) ((uint4 *)sB)[j] = ((const uint4 *)block)[j];
    if (t < FCX_SET_MAX_PATTERNS) sN[t] = 0;
    const uint64_t *sT0 = (const uint64_t *)(sB + kPsT0), *sT1 = (const uint64_t *)(sB + kPsT1);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15), rep = delim * 0x01010101u;
    // the tile, the M - 1 bytes behind it that a full compare reads, and one byte more: the filter reads the byte behind
    // every position, the tile's last one included (>= kSThreads + 1, <= kSPieces pieces)
    const uint32_t npieces = (kSTile + maxlen + 15) / 16;
    uint64_t judged = 0, cand = 0, compares = 0, nhits = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kSTile;
        __syncthreads();   // the readers of the tile before are done (the first round: sB and sN are there)
        uint4 raw = make_uint4(0, 0, 0, 0);   // this lane's 16 bytes before the fold: piece t, staged by thread t
        for (uint32_t j = t; j < npieces; j += kSThreads) {
            const uint64_t i = base + 16ull * j;
            uint4 w = make_uint4(0, 0, 0, 0);
            if (i + 16 <= len) {
                w = ld16_bounded(src, i, sh, len);
            } else if (i < len) {   // the range's last bytes
                uint32_t x[4] = {0, 0, 0, 0};
                for (uint32_t q = 0; q < (uint32_t)(len - i); q++) x[q >> 2] |= (uint32_t)src[i + q] << (8 * (q & 3));
                w = make_uint4(x[0], x[1], x[2], x[3]);
            }
            if (j == t) raw = w;
            if (fold) w = make_uint4(fold4(w.x), fold4(w.y), fold4(w.z), fold4(w.w));
            ((uint4 *)sT)[j] = w;
        }
        __syncthreads();
        const uint64_t at = base + kSPer * t;   // this lane's first position
        const uint32_t nj = at >= njudged ? 0u : (uint32_t)min((uint64_t)kSPer, njudged - at);
        const uint4 a = ((const uint4 *)sT)[t];
        uint32_t e = __shfl_down(a.x, 1, 64);
        if (lane == 63) e = sT[4 * t + 4];
        const uint32_t w[5] = {a.x, a.y, a.z, a.w, e};
        uint32_t c = 0;
#pragma unroll
        for (uint32_t b = 0; b < kSPer; b++) {
            const uint32_t v = __builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3);
            const uint64_t mk = sT0[v & 0xFFu] & sT1[(v >> 8) & 0xFFu];
            c |= (uint32_t)(mk != 0) << b;
        }
        c &= (1u << nj) - 1;
        judged += nj;
        cand += __popc(c);
        uint32_t hits = 0;
        while (c) {
            const uint32_t b = (uint32_t)__builtin_ctz(c);
            c &= c - 1;
            const uint32_t q = kSPer * t + b;
            const uint32_t v = __builtin_amdgcn_alignbyte(sT[(q >> 2) + 1], sT[q >> 2], q & 3);
            uint64_t mk = sT0[v & 0xFFu] & sT1[(v >> 8) & 0xFFu];
            const uint64_t room = len - (at + b);   // bytes from the position to the range's end (at + b < njudged <= len)
            bool any = false;
            while (mk) {
                const uint32_t k = (uint32_t)__builtin_ctzll(mk);
                mk &= mk - 1;
                const uint32_t meta = sB[kPsMeta + k], lk = meta & 0xFFFFu;
                if (lk > room) continue;
                if (lk > 2) {   // (one and two bytes: the tables have said it all)
                    compares++;
                    if (!set_full(sT, sB + kPsPat + (meta >> 16), q, lk)) continue;
                }
                atomicAdd(&sN[k], 1u);
                any = true;
            }
            if (any) hits |= 1u << b;
        }
        hit_bits[(uint64_t)tile * kSThreads + t] = (uint16_t)hits;
        uint32_t n = __popc(hits);
        if (GREP) {
            const uint32_t nb = at >= ndelim ? 0u : (uint32_t)min((uint64_t)kSPer, ndelim - at);
            uint32_t dl = set_eq_bits4(raw.x, rep) | set_eq_bits4(raw.y, rep) << 4 | set_eq_bits4(raw.z, rep) << 8 |
                          set_eq_bits4(raw.w, rep) << 12;
            dl &= (1u << nb) - 1;   // (the carried positions wait; bytes behind the range were loaded as zeros)
            delim_bits[(uint64_t)tile * kSThreads + t] = (uint16_t)dl;
            // the tile's summary: positions in the range, 1 + position
            const uint32_t at1 = (uint32_t)at + 1;
            uint32_t fd = dl ? at1 + (uint32_t)__builtin_ctz(dl) : kSNone;
            uint32_t ld = dl ? at1 + 31u - (uint32_t)__builtin_clz(dl) : 0u;
            uint32_t lh = hits ? at1 + 31u - (uint32_t)__builtin_clz(hits) : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                n += __shfl_xor(n, o, 64);
                fd = min(fd, (uint32_t)__shfl_xor(fd, o, 64));
                ld = max(ld, (uint32_t)__shfl_xor(ld, o, 64));
                lh = max(lh, (uint32_t)__shfl_xor(lh, o, 64));
            }
            if (lane == 0) {
                sR[4 * wv] = n;
                sR[4 * wv + 1] = fd;
                sR[4 * wv + 2] = ld;
                sR[4 * wv + 3] = lh;
            }
            __syncthreads();
            if (t == 0) {
                uint32_t tn = 0, tf = kSNone, tl = 0, th = 0;
                for (uint32_t q = 0; q < kSWaves; q++) {
                    tn += sR[4 * q];
                    tf = min(tf, sR[4 * q + 1]);
                    tl = max(tl, sR[4 * q + 2]);
                    th = max(th, sR[4 * q + 3]);
                }
                tile_out[kSSum * tile] = tn;
                tile_out[kSSum * tile + 1] = tf == kSNone ? 0u : tf;
                tile_out[kSSum * tile + 2] = tl;
                tile_out[kSSum * tile + 3] = th;
            }
        } else {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
            if (lane == 0) sR[wv] = n;
            __syncthreads();
            if (t == 0) tile_out[tile] = sR[0] + sR[1] + sR[2] + sR[3];
        }
        nhits += n;   // (uniform over the wave)
    }
    judged = wave_sum_u64(judged);
    cand = wave_sum_u64(cand);
    compares = wave_sum_u64(compares);
    if (lane == 0) {
        sJ[4 * wv] = judged;
        sJ[4 * wv + 1] = cand;
        sJ[4 * wv + 2] = compares;
        sJ[4 * wv + 3] = nhits;
    }
    __syncthreads();   // (and every lane's additions to sN are done)
    if (t == 0) {
        uint64_t s[4] = {0, 0, 0, 0};
        for (uint32_t q = 0; q < kSWaves; q++)
            for (uint32_t i = 0; i < 4; i++) s[i] += sJ[4 * q + i];
        unsigned long long *w = (unsigned long long *)swords;
        atomicAdd(w + kSwJudged, (unsigned long long)s[0]);
        if (s[1]) atomicAdd(w + kSwCand, (unsigned long long)s[1]);
        if (s[2]) atomicAdd(w + kSwCompares, (unsigned long long)s[2]);
        if (s[3]) atomicAdd(w + kSwHits, (unsigned long long)s[3]);
        atomicAdd((unsigned long long *)w_judged, (unsigned long long)s[0]);
        const uint64_t second = GREP ? s[3] : s[1];
        if (w_second && second) atomicAdd((unsigned long long *)w_second, (unsigned long long)second);
    }
    if (t < FCX_SET_MAX_PATTERNS && sN[t]) atomicAdd((unsigned long long *)swords + kSwCounts + t, (unsigned long long)sN[t]);
}

namespace {
const char *kSFStageNames[] = {"index", "decode", "scan", "summary"};
constexpr int kSFStages = 4;
const char *kSGStageNames[] = {"index", "decode", "scan", "select", "summary"};
constexpr int kSGStages = 5;

// the set's block to the device, and with `fresh` the counters of a new file
int ready_set(fcx_dctx *c, const fcx_pattern_set *set, bool fresh, hipStream_t st) {
    SetScratch &S = c->ps;
    if (!S.host_words) {
        FCX_TRY(S.block.reserve(4 * kPsWords, "pattern set"));
        FCX_TRY(S.words.reserve(8 * kSwWords, "pattern set words"));
        FCX_HIP(S.host_words.alloc(8 * kSwWords));
    }
    FCX_HIP(hipMemcpyAsync(S.block, set->block, 4 * kPsWords, hipMemcpyHostToDevice, st));
    if (fresh) {
        FCX_HIP(hipMemsetAsync(S.words, 0, 8 * kSwWords, st));
        for (uint64_t &v : S.stats) v = 0;
    }
    return FCX_OK;
}

// the scan counters and the per-pattern counts of the file so far (the caller synchronises, then calls set_publish)
int set_fetch(fcx_dctx *c, hipStream_t st) {
    SetScratch &S = c->ps;
    FCX_HIP(hipMemcpyAsync(S.host_words, S.words, 8 * kSwWords, hipMemcpyDeviceToHost, st));
    return FCX_OK;
}
void set_publish(fcx_dctx *c, const fcx_pattern_set *set, uint64_t *counts) {
    SetScratch &S = c->ps;
    for (int i = 0; i < 4; i++) S.stats[i] = S.host_words[i];
    for (uint32_t k = 0; k < set->npat && counts; k++) counts[k] = S.host_words[kSwCounts + k];
}

int ready_find(fcx_dctx *c) {   // (what fcx_find.hip's own calls set up: either may come first)
    FindScratch &F = c->fd;
    if (!F.host_words) {
        FCX_TRY(F.words.reserve(8 * kFwWords, "find words"));
        FCX_TRY(F.pat.reserve(kFCarry, "find pattern"));
        FCX_TRY(F.carry.reserve(kFCarry, "find carry"));
        FCX_HIP(F.host_words.alloc(8 * kFwWords));
    }
    return FCX_OK;
}

int ready_grep(fcx_dctx *c) {
    GrepScratch &G = c->gp;
    if (!G.host_words) {
        FCX_TRY(G.words.reserve(8 * kGwWords, "grep words"));
        FCX_TRY(G.pat.reserve(kFCarry, "grep pattern"));
        FCX_TRY(G.carry.reserve(kFCarry, "grep carry"));
        FCX_HIP(G.host_words.alloc(8 * kGwWords));
    }
    return FCX_OK;
}

int reserve_find_tiles(fcx_dctx *c, uint64_t range_bytes) {
    FindScratch &F = c->fd;
    const uint64_t tiles = (range_bytes + kSTile - 1) / kSTile + 1;
    FCX_TRY(F.bitmap.reserve(2ull * kSThreads * tiles, "find bitmap"));
    FCX_TRY(F.tile_count.reserve(4 * tiles, "find tile counts"));
    FCX_TRY(F.tile_base.reserve(4 * tiles, "find tile counts"));
    return FCX_OK;
}

int reserve_grep_tiles(fcx_dctx *c, uint64_t range_bytes) {
    GrepScratch &G = c->gp;
    const uint64_t tiles = (range_bytes + kSTile - 1) / kSTile + 1;
    FCX_TRY(G.hit_bits.reserve(2ull * kSThreads * tiles, "grep hit bits"));
    FCX_TRY(G.delim_bits.reserve(2ull * kSThreads * tiles, "grep delimiter bits"));
    FCX_TRY(G.tile_sum.reserve(4ull * kSSum * tiles, "grep tile words"));
    FCX_TRY(G.tile_ctx.reserve(8ull * kSCtx * tiles, "grep tile words"));
    FCX_TRY(G.tile_count.reserve(4 * tiles, "grep tile words"));
    FCX_TRY(G.tile_base.reserve(4 * tiles, "grep tile words"));
    G.scratch_bytes = std::max<uint64_t>(G.scratch_bytes, tiles * (4ull * kSThreads + 4 * kSSum + 8 * kSCtx + 8));
    return FCX_OK;
}

// positions of a range of len bytes that a scan judges: all that are left at the run's end, else those every pattern fits behind
uint64_t set_njudged(const fcx_pattern_set *set, uint64_t len, bool final) {
    const uint64_t need = final ? set->min_len : set->max_len;
    return len >= need ? len - need + 1 : 0;
}

// One range [src, src + len) of the search: scan, rank, the first cap hits and the windows of the stream form; the
// carry for the range behind it (none behind the final one).  pos_base: the file-wide offset of src[0].
int find_scan(fcx_dctx *c, const fcx_pattern_set *set, const uint8_t *src, uint64_t len, bool final, uint64_t pos_base,
              const FindSink &sink, uint64_t window, std::vector<uint64_t> *host_hits, hipStream_t st) {
    FindScratch &F = c->fd;
    SetScratch &S = c->ps;
    const uint64_t njudged = set_njudged(set, len, final);
    const uint32_t ntiles = (uint32_t)((njudged + kSTile - 1) / kSTile);
    const uint32_t grid = std::min(ntiles, kSMaxGrid);
    if (ntiles) {
        hipLaunchKernelGGL(k_sscan<false>, dim3(grid), dim3(kSThreads), 0, st, src, len, njudged, 0ull, set->max_len,
                           set->flags & FCX_SET_FOLD_ASCII, 0u, (const uint32_t *)S.block, ntiles, (uint16_t *)F.bitmap,
                           (uint16_t *)nullptr, (uint32_t *)F.tile_count, (uint64_t *)F.words + kFwJudged,
                           (uint64_t *)F.words + kFwCand, (uint64_t *)S.words);
        hipLaunchKernelGGL(k_fbase, dim3(1), dim3(kSBaseThreads), 0, st, (const uint32_t *)F.tile_count, ntiles,
                           (uint32_t *)F.tile_base, (uint64_t *)F.words);
        if (sink.cap)
            hipLaunchKernelGGL(k_fwrite, dim3(grid), dim3(kSThreads), 0, st, (const uint16_t *)F.bitmap,
                               (const uint32_t *)F.tile_count, (const uint32_t *)F.tile_base, ntiles, (const uint64_t *)F.words,
                               pos_base, 0ull, sink.cap, sink.d_hits);
    }
    FCX_HIP(hipGetLastError());
    const uint32_t keep = final ? 0u : (uint32_t)std::min<uint64_t>(set->max_len - 1, len);
    if (keep) hipLaunchKernelGGL(k_fcarry, dim3(1), dim3(kSThreads), 0, st, src, len, keep, (uint8_t *)F.carry);
    F.carry_len = keep;
    S.stats[4]++;
    if (final) S.stats[5]++;
    if (sink.on_hit && ntiles) {   // the range's hits, window after window of the same bitmap
        FCX_HIP(hipMemcpyAsync(F.host_words, F.words, 8 * kFwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        const uint64_t before = F.host_words[kFwGroupBase], end = F.host_words[kFwHits];
        for (uint64_t w0 = before; w0 < end; w0 += window) {
            const uint64_t n = std::min(window, end - w0);
            hipLaunchKernelGGL(k_fwrite, dim3(grid), dim3(kSThreads), 0, st, (const uint16_t *)F.bitmap,
                               (const uint32_t *)F.tile_count, (const uint32_t *)F.tile_base, ntiles, (const uint64_t *)F.words,
                               pos_base, w0, n, (uint64_t *)F.hits);
            FCX_HIP(hipGetLastError());
            host_hits->resize(n);
            FCX_HIP(hipMemcpyAsync(host_hits->data(), F.hits, 8 * n, hipMemcpyDeviceToHost, st));
            FCX_HIP(hipStreamSynchronize(st));
            for (uint64_t i = 0; i < n; i++) sink.on_hit(sink.user, (*host_hits)[i]);
        }
    }
    return FCX_OK;
}

// One range of the grep: scan, the select kernels, the first cap lines and the windows of the stream form with the
// open line held back; the carry for the range behind it.
int grep_scan(fcx_dctx *c, const fcx_pattern_set *set, uint8_t delim, const uint8_t *src, uint64_t len, bool final, uint64_t pos_base,
              const GrepSink &sink, GrepCarry *carry, uint64_t window, std::vector<uint64_t> *host_lines, RunTimes *T,
              hipStream_t st) {
    GrepScratch &G = c->gp;
    SetScratch &S = c->ps;
    // A group that is not the last contributes the positions every pattern fits behind, with their hit bits and
    // their delimiter bits alike: the M - 1 positions it carries are seen, as hits and as delimiters, by the range
    // behind it and by no other, so the select kernels see every position of the run exactly once.  The last
    // range contributes all its positions: a delimiter in it may close the open line where no pattern fits.
    const uint64_t njudged = set_njudged(set, len, final), ndelim = final ? len : njudged;
    const uint32_t ntiles = (uint32_t)((ndelim + kSTile - 1) / kSTile);
    const uint32_t grid = std::min(ntiles, kSMaxGrid);
    if (ntiles)
        hipLaunchKernelGGL(k_sscan<true>, dim3(grid), dim3(kSThreads), 0, st, src, len, njudged, ndelim, set->max_len,
                           set->flags & FCX_SET_FOLD_ASCII, (uint32_t)delim, (const uint32_t *)S.block, ntiles,
                           (uint16_t *)G.hit_bits, (uint16_t *)G.delim_bits, (uint32_t *)G.tile_sum,
                           (uint64_t *)G.words + kGwJudged, (uint64_t *)G.words + kGwHits, (uint64_t *)S.words);
    if (T) T->mark(3);
    if (ntiles) {
        hipLaunchKernelGGL(k_gtiles, dim3(1), dim3(kSBaseThreads), 0, st, (const uint32_t *)G.tile_sum, ntiles, pos_base,
                           (uint64_t *)G.tile_ctx, (uint64_t *)G.words, sink.d_end, sink.cap);
        hipLaunchKernelGGL(k_gmark, dim3(grid), dim3(kSThreads), 0, st, (uint16_t *)G.hit_bits, (const uint16_t *)G.delim_bits,
                           (const uint32_t *)G.tile_sum, (const uint64_t *)G.tile_ctx, ntiles, pos_base, (uint32_t *)G.tile_count,
                           (uint64_t *)G.words);
        hipLaunchKernelGGL(k_gbase, dim3(1), dim3(kSBaseThreads), 0, st, (const uint32_t *)G.tile_count, ntiles,
                           (uint32_t *)G.tile_base, (uint64_t *)G.words);
        if (sink.cap)
            hipLaunchKernelGGL(k_gwrite, dim3(grid), dim3(kSThreads), 0, st, (const uint16_t *)G.hit_bits,
                               (const uint16_t *)G.delim_bits, (const uint64_t *)G.tile_ctx, (const uint32_t *)G.tile_count,
                               (const uint32_t *)G.tile_base, ntiles, (const uint64_t *)G.words, pos_base, 0ull, sink.cap,
                               sink.d_start, sink.d_end);
    }
    if (T) T->mark(4);
    FCX_HIP(hipGetLastError());
    if (T) FCX_TRY(T->add(1, 4));
    const uint32_t keep = final ? 0u : (uint32_t)std::min<uint64_t>(set->max_len - 1, len);
    if (keep) hipLaunchKernelGGL(k_gcarry, dim3(1), dim3(kSThreads), 0, st, src, len, keep, (uint8_t *)G.carry);
    G.carry_len = keep;
    S.stats[4]++;
    if (final) S.stats[5]++;
    if (sink.on_line && carry && ntiles) {   // the range's lines, window after window of the same bitmaps
        FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        const uint64_t before = G.host_words[kGwGroupBase], end = G.host_words[kGwLines];
        const bool open = G.host_words[kGwOpen] != 0;
        if (carry->held && G.host_words[kGwClosed]) {   // the line held back has its end
            sink.on_line(sink.user, carry->held_start, G.host_words[kGwClosed]);
            carry->held = false;
        }
        for (uint64_t w0 = before; w0 < end; w0 += window) {
            const uint64_t n = std::min(window, end - w0);
            hipLaunchKernelGGL(k_gwrite, dim3(grid), dim3(kSThreads), 0, st, (const uint16_t *)G.hit_bits,
                               (const uint16_t *)G.delim_bits, (const uint64_t *)G.tile_ctx, (const uint32_t *)G.tile_count,
                               (const uint32_t *)G.tile_base, ntiles, (const uint64_t *)G.words, pos_base, w0, n,
                               (uint64_t *)G.win_start, (uint64_t *)G.win_end);
            FCX_HIP(hipGetLastError());
            host_lines->resize(2 * n);
            FCX_HIP(hipMemcpyAsync(host_lines->data(), G.win_start, 8 * n, hipMemcpyDeviceToHost, st));
            FCX_HIP(hipMemcpyAsync(host_lines->data() + n, G.win_end, 8 * n, hipMemcpyDeviceToHost, st));
            FCX_HIP(hipStreamSynchronize(st));
            for (uint64_t i = 0; i < n; i++) {
                if (open && w0 + i + 1 == end) {   // the range's last line is still open: its end is to come
                    carry->held = true;
                    carry->held_start = (*host_lines)[i];
                } else {
                    sink.on_line(sink.user, (*host_lines)[i], (*host_lines)[n + i]);
                }
            }
        }
    }
    return FCX_OK;
}

// the grep's five stats from its words (the caller has synchronised)
void grep_stats_out(fcx_dctx *c, uint64_t total, uint64_t *stats) {
    GrepScratch &G = c->gp;
    stats[0] = G.host_words[kGwLines];
    stats[1] = G.host_words[kGwBytes];
    stats[2] = G.host_words[kGwHits];
    stats[3] = G.host_words[kGwJudged];
    stats[4] = total;
}
}  // namespace

int set_args(const char *fn, const fcx_pattern_set *set, int delim) {
    if (!set || set->npat < 1 || set->npat > FCX_SET_MAX_PATTERNS) return fail(FCX_ERR_ARG, std::string(fn) + ": not a pattern set");
    if (delim < 0) return FCX_OK;
    if (set->holds((uint8_t)delim)) return fail(FCX_ERR_ARG, std::string(fn) + ": a pattern holds the delimiter");
    if ((set->flags & FCX_SET_FOLD_ASCII) && set->holds(fold_ascii((uint8_t)delim)))
        return fail(FCX_ERR_ARG, std::string(fn) + ": a folded pattern holds the folded delimiter");
    return FCX_OK;
}

// ---- what the blocks calls (fcx_context.hip) take from here: the one scan path and its scratch ----
int context_ready(fcx_dctx *c, const fcx_pattern_set *set, bool fresh, hipStream_t st) {
    FCX_TRY(ready_grep(c));
    return ready_set(c, set, fresh, st);
}
int context_reserve(fcx_dctx *c, uint64_t range_bytes) { return reserve_grep_tiles(c, range_bytes); }
int context_scan(fcx_dctx *c, const fcx_pattern_set *set, uint8_t delim, const uint8_t *src, uint64_t len, bool final,
                 uint32_t *ntiles, hipStream_t st) {
    GrepScratch &G = c->gp;
    SetScratch &S = c->ps;
    // (grep_scan's rule: hit bits and delimiter bits over the same positions, each seen by exactly one range)
    const uint64_t njudged = set_njudged(set, len, final), ndelim = final ? len : njudged;
    *ntiles = (uint32_t)((ndelim + kSTile - 1) / kSTile);
    if (*ntiles)
        hipLaunchKernelGGL(k_sscan<true>, dim3(std::min(*ntiles, kSMaxGrid)), dim3(kSThreads), 0, st, src, len, njudged, ndelim,
                           set->max_len, set->flags & FCX_SET_FOLD_ASCII, (uint32_t)delim, (const uint32_t *)S.block, *ntiles,
                           (uint16_t *)G.hit_bits, (uint16_t *)G.delim_bits, (uint32_t *)G.tile_sum, (uint64_t *)G.words + kGwJudged,
                           (uint64_t *)G.words + kGwHits, (uint64_t *)S.words);
    S.stats[4]++;
    if (final) S.stats[5]++;
    return FCX_OK;
}
int context_fetch(fcx_dctx *c, hipStream_t st) { return set_fetch(c, st); }
void context_publish(fcx_dctx *c, const fcx_pattern_set *set, uint64_t *counts) { set_publish(c, set, counts); }

int find_set_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_pattern_set *set,
                 uint64_t base, const FindSink &sink, bool last, uint64_t *nhits, uint64_t *decoded, uint64_t *counts, hipStream_t st,
                 uint64_t rec_base) {
    const bool fresh = rec_base == 0;   // (a file's first run: a new search)
    *nhits = 0;
    if (decoded) *decoded = 0;
    if (fresh) {
        c->fd.carry_len = 0;
        for (uint64_t &v : c->ps.stats) v = 0;
        for (uint32_t k = 0; k < set->npat && counts; k++) counts[k] = 0;
    }
    if (nblocks == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready_find(c));
    FindScratch &F = c->fd;
    VerifyScratch &V = c->vf;
    const uint64_t window = F.window ? F.window : kSWindow;
    if (sink.on_hit) FCX_TRY(F.hits.reserve(8 * window, "find hits"));
    RunTimes T(c, kSFStages, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    FCX_TRY(ready_set(c, set, fresh, st));
    FCX_HIP(hipMemsetAsync(F.words, 0, 8 * kFwWords, st));
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host)
    const std::vector<uint64_t> &doff = ix.doff;
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups, nullptr, kFCarry));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most + kFCarry > kSMaxRange)
        return fail(FCX_ERR_ARG, "fcx_find_set_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    FCX_TRY(reserve_find_tiles(c, most + kFCarry));
    std::vector<uint64_t> host_hits;
    uint8_t *const dec = V.buf + kFCarry;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const RunGroup &g = groups[gi];
        const uint32_t cl = F.carry_len;
        if (cl) FCX_HIP(hipMemcpyAsync(dec - cl, F.carry + (kFCarry - cl), cl, hipMemcpyDeviceToDevice, st));
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, dec, g.gbytes, st, rec_base, "fcx_find_set_shard"));
        T.mark(2);
        FCX_TRY(find_scan(c, set, dec - cl, cl + g.gbytes, last && gi + 1 == groups.size(), base + doff[g.g0] - cl, sink, window,
                          &host_hits, st));
        T.mark(3);
        FCX_TRY(T.add(1, 3));
    }
    T.mark(3);
    FCX_HIP(hipMemcpyAsync(F.host_words, F.words, 8 * kFwWords, hipMemcpyDeviceToHost, st));
    FCX_TRY(set_fetch(c, st));
    T.mark(4);
    FCX_HIP(hipStreamSynchronize(st));
    set_publish(c, set, counts);
    *nhits = F.host_words[kFwHits];
    if (decoded) *decoded = doff[nblocks];
    FCX_TRY(T.add(3, 4));
    T.publish(c, kSFStageNames, kSFStages);
    return FCX_OK;
}

int find_set_final(fcx_dctx *c, const fcx_pattern_set *set, uint64_t total, const FindSink &sink, uint64_t *nhits, uint64_t *counts,
                   hipStream_t st) {
    *nhits = 0;
    FindScratch &F = c->fd;
    const uint32_t cl = F.carry_len;
    if (cl == 0) {   // nothing is left to judge (M == 1, or nothing was decoded): the end is a final pass all the same
        c->ps.stats[5]++;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    const uint64_t window = F.window ? F.window : kSWindow;
    FCX_TRY(reserve_find_tiles(c, kFCarry));
    FCX_HIP(hipMemsetAsync(F.words, 0, 8 * kFwWords, st));
    std::vector<uint64_t> host_hits;
    FCX_TRY(find_scan(c, set, (const uint8_t *)F.carry + (kFCarry - cl), cl, true, total - cl, sink, window, &host_hits, st));
    FCX_HIP(hipMemcpyAsync(F.host_words, F.words, 8 * kFwWords, hipMemcpyDeviceToHost, st));
    FCX_TRY(set_fetch(c, st));
    FCX_HIP(hipStreamSynchronize(st));
    set_publish(c, set, counts);
    *nhits = F.host_words[kFwHits];
    return FCX_OK;
}

int grep_set_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                 const fcx_pattern_set *set, const GrepSink &sink, GrepCarry *carry, uint64_t *stats, uint64_t *counts, hipStream_t st,
                 uint64_t rec_base) {
    const bool fresh = !carry || carry->base == 0;   // (nothing was seen before a run at offset 0)
    if (fresh) {
        for (int i = 0; i < FCX_GREP_STATS; i++) stats[i] = 0;
        c->gp.scratch_bytes = 0;
        for (uint64_t &v : c->ps.stats) v = 0;
        for (uint32_t k = 0; k < set->npat && counts; k++) counts[k] = 0;
    }
    if (nblocks == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready_grep(c));
    GrepScratch &G = c->gp;
    VerifyScratch &V = c->vf;
    const uint64_t window = c->fd.window ? c->fd.window : kSWindow;
    if (sink.on_line) {
        FCX_TRY(G.win_start.reserve(8 * window, "grep lines"));
        FCX_TRY(G.win_end.reserve(8 * window, "grep lines"));
    }
    RunTimes T(c, kSGStages, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    FCX_TRY(ready_set(c, set, fresh, st));
    if (fresh) {
        FCX_HIP(hipMemsetAsync(G.words, 0, 8 * kGwWords, st));
        G.carry_len = 0;
    }
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host)
    const std::vector<uint64_t> &doff = ix.doff;
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups, nullptr, kFCarry));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most + kFCarry > kSMaxRange)
        return fail(FCX_ERR_ARG, "fcx_grep_set_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    FCX_TRY(reserve_grep_tiles(c, most + kFCarry));
    const uint64_t base = carry ? carry->base : 0, total = base + doff[nblocks];
    std::vector<uint64_t> host_lines;
    uint8_t *const dec = V.buf + kFCarry;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const RunGroup &g = groups[gi];
        const uint32_t cl = G.carry_len;
        if (cl) FCX_HIP(hipMemcpyAsync(dec - cl, G.carry + (kFCarry - cl), cl, hipMemcpyDeviceToDevice, st));
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, dec, g.gbytes, st, rec_base, "fcx_grep_set_shard"));
        T.mark(2);
        FCX_TRY(grep_scan(c, set, delim, dec - cl, cl + g.gbytes, !carry && gi + 1 == groups.size(), base + doff[g.g0] - cl, sink,
                          carry, window, &host_lines, &T, st));
    }
    T.mark(4);
    if (!carry) hipLaunchKernelGGL(k_gfinish, dim3(1), dim3(1), 0, st, (uint64_t *)G.words, total, sink.d_end, sink.cap);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
    FCX_TRY(set_fetch(c, st));
    T.mark(5);
    FCX_HIP(hipStreamSynchronize(st));
    set_publish(c, set, counts);
    grep_stats_out(c, total, stats);
    if (carry) carry->base = total;
    FCX_TRY(T.add(4, 5));
    T.publish(c, kSGStageNames, kSGStages);
    return FCX_OK;
}

int grep_set_final(fcx_dctx *c, uint8_t delim, const fcx_pattern_set *set, const GrepSink &sink, GrepCarry *carry, uint64_t *stats,
                   uint64_t *counts, hipStream_t st) {
    GrepScratch &G = c->gp;
    const uint32_t cl = G.carry_len;
    if (cl == 0 || carry->base == 0) {   // nothing is left to judge: the end is a final pass all the same
        c->ps.stats[5]++;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    const uint64_t window = c->fd.window ? c->fd.window : kSWindow;
    FCX_TRY(reserve_grep_tiles(c, kFCarry));
    std::vector<uint64_t> host_lines;
    FCX_TRY(grep_scan(c, set, delim, (const uint8_t *)G.carry + (kFCarry - cl), cl, true, carry->base - cl, sink, carry, window,
                      &host_lines, nullptr, st));
    FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
    FCX_TRY(set_fetch(c, st));
    FCX_HIP(hipStreamSynchronize(st));
    set_publish(c, set, counts);
    grep_stats_out(c, carry->base, stats);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_pattern_set_create(fcx_pattern_set **set, const uint8_t *bytes, const uint32_t *lens, uint32_t npat, uint32_t flags) {
    if (!set) return fail(FCX_ERR_ARG, "fcx_pattern_set_create: NULL argument");
    *set = nullptr;
    fcx_pattern_set *s = new (std::nothrow) fcx_pattern_set();
    if (!s) return fail(FCX_ERR_NOMEM, "fcx_pattern_set_create: out of memory");
    if (const char *why = patset_compile(s, bytes, lens, npat, flags)) {
        delete s;
        return fail(FCX_ERR_ARG, std::string("fcx_pattern_set_create: ") + why);
    }
    *set = s;
    return FCX_OK;
}

void fcx_pattern_set_destroy(fcx_pattern_set *set) { delete set; }

int fcx_pattern_set_info(const fcx_pattern_set *set, uint32_t *npat, uint32_t *min_len, uint32_t *max_len, uint32_t *flags) {
    if (!set) return fail(FCX_ERR_ARG, "fcx_pattern_set_info: NULL set");
    if (npat) *npat = set->npat;
    if (min_len) *min_len = set->min_len;
    if (max_len) *max_len = set->max_len;
    if (flags) *flags = set->flags;
    return FCX_OK;
}

int fcx_find_set_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_pattern_set *set,
                       uint64_t *d_hits, uint64_t cap, uint64_t *nhits, uint64_t *counts, void *stream) {
    if (!c || !set || !nhits || (nblocks && !d_rec) || (cap && !d_hits))
        return fail(FCX_ERR_ARG, "fcx_find_set_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_find_set_shard: kind must be '7' or '8'");
    FCX_TRY(set_args("fcx_find_set_shard", set, -1));
    FindSink sink;
    sink.d_hits = d_hits;
    sink.cap = cap;
    return find_set_run(c, kind, d_rec, rec_len, nblocks, set, 0, sink, true, nhits, nullptr, counts, (hipStream_t)stream, 0);
}

int fcx_grep_set_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                       const fcx_pattern_set *set, uint64_t *d_start, uint64_t *d_end, uint64_t cap, uint64_t *stats, uint64_t *counts,
                       void *stream) {
    if (!c || !set || !stats || (nblocks && !d_rec) || (cap && (!d_start || !d_end)))
        return fail(FCX_ERR_ARG, "fcx_grep_set_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_grep_set_shard: kind must be '7' or '8'");
    FCX_TRY(set_args("fcx_grep_set_shard", set, delim));
    GrepSink sink;
    sink.d_start = d_start;
    sink.d_end = d_end;
    sink.cap = cap;
    return grep_set_run(c, kind, d_rec, rec_len, nblocks, delim, set, sink, nullptr, stats, counts, (hipStream_t)stream, 0);
}

int fcx_dctx_set_scan_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_set_scan_stats: bad argument");
    for (int i = 0; i < n && i < FCX_SET_SCAN_STATS; i++) out[i] = c->ps.stats[i];
    return FCX_OK;
}

}  // extern "C"
