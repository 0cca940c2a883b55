// fcx_grep.hip — matching lines of a device-resident run (gfx950): which lines of what the records decode to
// hold a byte string?  fcx_grep_shard of include/fcx.h (its host form: fcx_ranges.hip).  DESIGN.md §9i.
//
//   the run      on the run core as the search's: index, then per record group the decode to
//                buf + kFCarry with the carry of m - 1 bytes in front, so [carry | group] is one byte range.
//                What goes from group to group beside the carry is the status words kGw*: the last delimiter,
//                the last hit, the lines so far and whether the open line is selected; positions are run-wide
//                and kept as 1 + position, 0 meaning none.  The delimiters of the carry are seen twice, which
//                changes nothing: every use of a delimiter is a maximum or a minimum over positions.
//   k_gscan      k_fscan's tile shape (256 lanes, 4096 start positions, the tile and its halo in LDS through
//                ld16_bounded): 16 hit bits and 16 delimiter bits per lane, and per tile its hits, its first
//                and last delimiter and its last hit.
//   k_gtiles     one workgroup over the tile summaries, seeded with the carried words: a forward maximum scan
//                gives each tile the last delimiter and the last hit before it, a backward minimum scan the
//                first delimiter behind it.  It closes the line the group before left open (its end is the
//                group's first delimiter) and leaves the words for the next group.
//   k_gmark      per tile: a hit is the first of its line iff the hit before it lies in front of the line's
//                start.  The hit bits become first-hit bits, counted per tile; the lines' bytes are summed.
//   k_gbase      one workgroup: the exclusive scan of the tile counts, and the call's lines so far.
//   k_gwrite     per tile whose ranks lie below cap: start = 1 + the last delimiter before the hit, end = 1 +
//                the first delimiter behind it, to d_start / d_end[rank]; an end the group does not hold is
//                left to k_gtiles of a later group or to k_gfinish (the run's end).  The stream form calls it
//                once per window of lines, over the same bitmaps.
// Nothing here is proportional to the hits or the lines: two bitmaps and 48 bytes per tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"

namespace fcx {

constexpr uint32_t kGThreads = 256;
constexpr uint32_t kGWaves = kGThreads / 64;
constexpr uint32_t kGPer = 16;                                // positions per lane
constexpr uint32_t kGTile = kGPer * kGThreads;                // positions per tile (4096)
constexpr uint32_t kGPieces = (kGTile + kFCarry + 15) / 16;   // 16-byte pieces of a tile and its halo at most
constexpr uint32_t kGLdsBytes = 16 * kGPieces + 16;           // (+ 16: the dword behind the last lane's bytes)
constexpr uint32_t kGMaxGrid = 2048;
constexpr uint32_t kGBaseThreads = 1024;
constexpr uint64_t kGMaxRange = 0xFFFF0000ull;                // bytes of [carry | group] at most
constexpr uint32_t kGNone = 0xFFFFFFFFu;
constexpr uint32_t kGWindow = 1u << 20;                       // lines per window of the stream form by default
constexpr uint32_t kGSum = 4, kGCtx = 3;                      // words per tile of tile_sum / tile_ctx

// bytes [4, m) of the pattern against the LDS bytes at q + 4 ... (the first 4 passed the filter)
__device__ inline bool grep_rest(const uint32_t *sT, const uint32_t *sP, uint32_t q, uint32_t m) {
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

// bit q of the result: byte q of the dword equals the byte replicated in rep (the carry-free zero-byte form)
__device__ inline uint32_t eq_bits4(uint32_t x, uint32_t rep) {
    x ^= rep;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// The range [src, src + len): bit p & 15 of hit_bits[p >> 4] says whether src[p, p + m) is the pattern, for
// p < njudged = len - m + 1; of delim_bits, whether src[p] is the delimiter, for p < len.  tile_sum[4 k ..]:
// the tile's hits, 1 + its first delimiter, 1 + its last delimiter, 1 + its last hit (positions in the range,
// 0: none).  words: kGwJudged and kGwHits advance.
__global__ __launch_bounds__(kGThreads) void k_gscan(const uint8_t *__restrict__ src, uint64_t len, uint64_t njudged, uint32_t m,
                                                     uint32_t delim, const uint32_t *__restrict__ pat, uint32_t ntiles,
                                                     uint16_t *__restrict__ hit_bits, uint16_t *__restrict__ delim_bits,
                                                     uint32_t *__restrict__ tile_sum, uint64_t *__restrict__ words) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kGLdsBytes / 4];
    __shared__ uint32_t sP[kFCarry / 4];
    __shared__ uint32_t sR[4 * kGWaves];
    __shared__ uint64_t sJ[2 * kGWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t < kFCarry / 4) sP[t] = pat[t];
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15), rep = delim * 0x01010101u;
    const uint32_t pmask = m >= 4 ? 0xFFFFFFFFu : (1u << (8 * m)) - 1, p0 = pat[0] & pmask;
    const uint32_t npieces = (kGTile + m - 1 + 15) / 16;   // (<= kGPieces)
    uint64_t judged = 0, nhits = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kGTile;
        __syncthreads();   // the readers of the tile before are done (the first round: sP is there)
        for (uint32_t j = t; j < npieces; j += kGThreads) {
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
        const uint64_t at = base + kGPer * t;   // this lane's first position
        const uint32_t nj = at >= njudged ? 0u : (uint32_t)min((uint64_t)kGPer, njudged - at);
        const uint32_t nb = at >= len ? 0u : (uint32_t)min((uint64_t)kGPer, len - at);
        const uint4 a = ((const uint4 *)sT)[t];
        uint32_t e = __shfl_down(a.x, 1, 64);
        if (lane == 63) e = sT[4 * t + 4];
        const uint32_t w[5] = {a.x, a.y, a.z, a.w, e};
        uint32_t c = 0;
#pragma unroll
        for (uint32_t b = 0; b < kGPer; b++) {
            const uint32_t v = __builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3);
            c |= (uint32_t)(((v ^ p0) & pmask) == 0) << b;
        }
        c &= (1u << nj) - 1;
        judged += nj;
        uint32_t hits = c;
        if (m > 4) {
            hits = 0;
            while (c) {
                const uint32_t b = (uint32_t)__builtin_ctz(c);
                c &= c - 1;
                if (grep_rest(sT, sP, kGPer * t + b, m)) hits |= 1u << b;
            }
        }
        uint32_t dl = eq_bits4(a.x, rep) | eq_bits4(a.y, rep) << 4 | eq_bits4(a.z, rep) << 8 | eq_bits4(a.w, rep) << 12;
        dl &= (1u << nb) - 1;   // (bytes behind the range were loaded as zeros)
        hit_bits[(uint64_t)tile * kGThreads + t] = (uint16_t)hits;
        delim_bits[(uint64_t)tile * kGThreads + t] = (uint16_t)dl;
        // the tile's summary: positions in the range, 1 + position
        const uint32_t at1 = (uint32_t)at + 1;
        uint32_t n = __popc(hits);
        uint32_t fd = dl ? at1 + (uint32_t)__builtin_ctz(dl) : kGNone;
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
            uint32_t tn = 0, tf = kGNone, tl = 0, th = 0;
            for (uint32_t q = 0; q < kGWaves; q++) {
                tn += sR[4 * q];
                tf = min(tf, sR[4 * q + 1]);
                tl = max(tl, sR[4 * q + 2]);
                th = max(th, sR[4 * q + 3]);
            }
            tile_sum[kGSum * tile] = tn;
            tile_sum[kGSum * tile + 1] = tf == kGNone ? 0u : tf;
            tile_sum[kGSum * tile + 2] = tl;
            tile_sum[kGSum * tile + 3] = th;
        }
        nhits += n;   // (uniform over the wave)
    }
    judged = wave_sum_u64(judged);
    if (lane == 0) {
        sJ[2 * wv] = judged;
        sJ[2 * wv + 1] = nhits;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long *w = (unsigned long long *)words;
        uint64_t j = 0, h = 0;
        for (uint32_t q = 0; q < kGWaves; q++) {
            j += sJ[2 * q];
            h += sJ[2 * q + 1];
        }
        atomicAdd(w + kGwJudged, (unsigned long long)j);
        if (h) atomicAdd(w + kGwHits, (unsigned long long)h);
    }
}

// block-wide exclusive maximum scan, forwards (blockDim.x threads, <= 16 waves); the maximum of all in *all
__device__ inline uint32_t block_xmax(uint32_t v, uint32_t *sh, uint32_t *all) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc = max(inc, u);
    }
    if (lane == 63) sh[wv] = inc;
    uint32_t pre = __shfl_up(inc, 1, 64);
    if (lane == 0) pre = 0;
    __syncthreads();
    uint32_t a = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t x = sh[w];
        if (w < wv) pre = max(pre, x);
        a = max(a, x);
    }
    __syncthreads();
    *all = a;
    return pre;
}

// block-wide exclusive minimum scan, backwards: the minimum over the threads behind this one (kGNone: none)
__device__ inline uint32_t block_xmin_back(uint32_t v, uint32_t *sh, uint32_t *all) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_down(inc, o, 64);
        if (lane + (uint32_t)o < 64) inc = min(inc, u);
    }
    if (lane == 0) sh[wv] = inc;
    uint32_t suf = __shfl_down(inc, 1, 64);
    if (lane == 63) suf = kGNone;
    __syncthreads();
    uint32_t a = kGNone;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t x = sh[w];
        if (w > wv) suf = min(suf, x);
        a = min(a, x);
    }
    __syncthreads();
    *all = a;
    return suf;
}

// One workgroup.  tile_ctx[3 k ..] = 1 + the last delimiter before tile k, 1 + the last hit before it, 1 + the
// first delimiter behind it, run-wide (0: none; the first two reach back through the carried words).  The line
// the group before left open ends at this group's first delimiter: into d_end[lines - 1] when that slot lies
// below cap, its bytes to kGwBytes, the end itself to kGwClosed (0: no line was closed).  words: kGwLast,
// kGwLastHit and kGwOpen as the group leaves them.
// pos_base: the run-wide offset of the range's first byte.
__global__ __launch_bounds__(kGBaseThreads) void k_gtiles(const uint32_t *__restrict__ tile_sum, uint32_t ntiles, uint64_t pos_base,
                                                          uint64_t *__restrict__ tile_ctx, uint64_t *__restrict__ words,
                                                          uint64_t *__restrict__ d_end, uint64_t cap) {
    __shared__ uint32_t sh[kGBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (ntiles + kGBaseThreads - 1) / kGBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    const uint64_t last0 = words[kGwLast], hit0 = words[kGwLastHit], open0 = words[kGwOpen], lines0 = words[kGwLines];
    uint32_t a_ld = 0, a_lh = 0, a_fd = kGNone;
    for (uint32_t k = k0; k < k1; k++) {
        const uint32_t fd = tile_sum[kGSum * k + 1];
        a_ld = max(a_ld, tile_sum[kGSum * k + 2]);
        a_lh = max(a_lh, tile_sum[kGSum * k + 3]);
        if (fd && a_fd == kGNone) a_fd = fd;
    }
    uint32_t g_ld, g_lh, g_fd;
    uint32_t ld = block_xmax(a_ld, sh, &g_ld);
    uint32_t lh = block_xmax(a_lh, sh, &g_lh);
    uint32_t nd = block_xmin_back(a_fd, sh, &g_fd);
    for (uint32_t k = k0; k < k1; k++) {
        tile_ctx[kGCtx * k] = ld ? pos_base + ld : last0;
        tile_ctx[kGCtx * k + 1] = lh ? pos_base + lh : hit0;
        ld = max(ld, tile_sum[kGSum * k + 2]);
        lh = max(lh, tile_sum[kGSum * k + 3]);
    }
    for (uint32_t k = k1; k > k0; k--) {
        tile_ctx[kGCtx * (k - 1) + 2] = nd != kGNone ? pos_base + nd : 0ull;
        const uint32_t fd = tile_sum[kGSum * (k - 1) + 1];
        if (fd) nd = fd;
    }
    if (t == 0) {   // (every thread has read the words: the scans synchronised)
        uint64_t closed = 0;
        if (open0 && g_fd != kGNone) {
            closed = pos_base + g_fd;
            if (lines0 - 1 < cap) d_end[lines0 - 1] = closed;
            words[kGwBytes] += closed - last0;
        }
        words[kGwClosed] = closed;
        const uint64_t last = g_ld ? max(last0, pos_base + g_ld) : last0, hit = g_lh ? max(hit0, pos_base + g_lh) : hit0;
        words[kGwLast] = last;
        words[kGwLastHit] = hit;
        words[kGwOpen] = hit > last ? 1 : 0;
    }
}

// What a lane of a tile knows of its surroundings, run-wide and as 1 + position (0: none): the last delimiter and
// the last hit in front of its 16 positions, the first delimiter behind them.  Within the wave by ballot and one
// shuffle from the nearest lane that has a bit, across the waves through LDS, beyond the tile from tile_ctx.
// Every thread of the workgroup calls it (it synchronises); sW: 3 * kGWaves words.
struct LaneCtx {
    uint64_t ld, lh, nd;
};
__device__ inline LaneCtx lane_ctx(uint32_t h, uint32_t dl, uint64_t tile1, const uint64_t *__restrict__ ctx, uint32_t *sW) {
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t v_ld = dl ? kGPer * t + 32u - (uint32_t)__builtin_clz(dl) : 0u;   // 1 + position in the tile
    const uint32_t v_lh = h ? kGPer * t + 32u - (uint32_t)__builtin_clz(h) : 0u;
    const uint32_t v_nd = dl ? kGPer * t + 1u + (uint32_t)__builtin_ctz(dl) : 0u;
    const uint64_t md = __ballot(dl != 0), mh = __ballot(h != 0), below = (1ull << lane) - 1, above = ~((2ull << lane) - 1);
    uint32_t ld = __shfl(v_ld, (md & below) ? 63 - __builtin_clzll(md & below) : 0, 64);
    uint32_t lh = __shfl(v_lh, (mh & below) ? 63 - __builtin_clzll(mh & below) : 0, 64);
    uint32_t nd = __shfl(v_nd, (md & above) ? __builtin_ctzll(md & above) : 0, 64);
    if (!(md & below)) ld = 0;
    if (!(mh & below)) lh = 0;
    if (!(md & above)) nd = 0;
    const uint32_t w_ld = __shfl(v_ld, md ? 63 - __builtin_clzll(md) : 0, 64);
    const uint32_t w_lh = __shfl(v_lh, mh ? 63 - __builtin_clzll(mh) : 0, 64);
    const uint32_t w_nd = __shfl(v_nd, md ? __builtin_ctzll(md) : 0, 64);
    __syncthreads();   // sW of the tile before is read
    if (lane == 0) {
        sW[3 * wv] = md ? w_ld : 0u;
        sW[3 * wv + 1] = mh ? w_lh : 0u;
        sW[3 * wv + 2] = md ? w_nd : 0u;
    }
    __syncthreads();
    for (uint32_t q = 0; q < wv; q++) {
        ld = max(ld, sW[3 * q]);
        lh = max(lh, sW[3 * q + 1]);
    }
    for (uint32_t q = wv + 1; q < kGWaves; q++)
        if (!nd) nd = sW[3 * q + 2];
    LaneCtx r;
    r.ld = ld ? tile1 - 1 + ld : ctx[0];
    r.lh = lh ? tile1 - 1 + lh : ctx[1];
    r.nd = nd ? tile1 - 1 + nd : ctx[2];
    return r;
}

// 1 + the first delimiter behind bit b of a lane (run-wide; 0: the group holds none): base1 = 1 + the run-wide
// position of the lane's bit 0
__device__ inline uint64_t end_behind(uint32_t dl, uint32_t b, uint64_t base1, uint64_t nd) {
    const uint32_t rest = dl & ~((2u << b) - 1);
    return rest ? base1 + (uint32_t)__builtin_ctz(rest) : nd;
}

// hit_bits: the hits become the first hits of their lines; tile_count[k]: those of tile k; words: kGwBytes
// advances by end - start of every line that starts being selected here and ends in the group.
__global__ __launch_bounds__(kGThreads) void k_gmark(uint16_t *__restrict__ hit_bits, const uint16_t *__restrict__ delim_bits,
                                                     const uint32_t *__restrict__ tile_sum, const uint64_t *__restrict__ tile_ctx,
                                                     uint32_t ntiles, uint64_t pos_base, uint32_t *__restrict__ tile_count,
                                                     uint64_t *__restrict__ words) {
    __shared__ uint32_t sW[3 * kGWaves];
    __shared__ uint32_t sC[kGWaves];
    __shared__ uint64_t sB[kGWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint64_t bytes = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tile_sum[kGSum * tile] == 0) {   // (the whole workgroup) no hit, no line
            if (t == 0) tile_count[tile] = 0;
            continue;
        }
        const uint32_t h = hit_bits[(uint64_t)tile * kGThreads + t], dl = delim_bits[(uint64_t)tile * kGThreads + t];
        const uint64_t tile1 = pos_base + (uint64_t)tile * kGTile + 1;
        const LaneCtx c = lane_ctx(h, dl, tile1, tile_ctx + kGCtx * (uint64_t)tile, sW);
        const uint64_t base1 = tile1 + kGPer * t;
        uint64_t ld = c.ld, ph = c.lh;
        uint32_t u = h | dl, first = 0;
        while (u) {
            const uint32_t b = (uint32_t)__builtin_ctz(u);
            u &= u - 1;
            if ((dl >> b) & 1) {
                ld = base1 + b;
                continue;
            }
            if (ph <= ld) {   // the hit before lies in front of the line's start (or there is none)
                first |= 1u << b;
                const uint64_t end = end_behind(dl, b, base1, c.nd);
                if (end) bytes += end - ld;
            }
            ph = base1 + b;
        }
        hit_bits[(uint64_t)tile * kGThreads + t] = (uint16_t)first;
        uint32_t n = __popc(first);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) sC[wv] = n;
        __syncthreads();
        if (t == 0) tile_count[tile] = sC[0] + sC[1] + sC[2] + sC[3];
    }
    bytes = wave_sum_u64(bytes);
    if (lane == 0) sB[wv] = bytes;
    __syncthreads();
    if (t == 0 && sB[0] + sB[1] + sB[2] + sB[3])
        atomicAdd((unsigned long long *)words + kGwBytes, (unsigned long long)(sB[0] + sB[1] + sB[2] + sB[3]));
}

// One workgroup: tile_base[k] = first hits of the group's tiles before k; words: kGwGroupBase = the call's lines
// before this group, kGwLines advanced by the group's.
__global__ __launch_bounds__(kGBaseThreads) void k_gbase(const uint32_t *__restrict__ tile_count, uint32_t ntiles,
                                                         uint32_t *__restrict__ tile_base, uint64_t *__restrict__ words) {
    __shared__ uint32_t sh[kGBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (ntiles + kGBaseThreads - 1) / kGBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    uint32_t s = 0, tot;
    for (uint32_t k = k0; k < k1; k++) s += tile_count[k];
    uint32_t run = block_xscan(s, sh, &tot);
    for (uint32_t k = k0; k < k1; k++) {
        tile_base[k] = run;
        run += tile_count[k];
    }
    if (t == 0) {
        const uint64_t before = words[kGwLines];
        words[kGwGroupBase] = before;
        words[kGwLines] = before + tot;
    }
}

// The lines that start being selected in the group and whose rank in the call lies in [win0, win0 + winlen): start
// and end to d_start / d_end[rank - win0]; an end behind the group stays unwritten here.
__global__ __launch_bounds__(kGThreads) void k_gwrite(const uint16_t *__restrict__ hit_bits, const uint16_t *__restrict__ delim_bits,
                                                      const uint64_t *__restrict__ tile_ctx, const uint32_t *__restrict__ tile_count,
                                                      const uint32_t *__restrict__ tile_base, uint32_t ntiles,
                                                      const uint64_t *__restrict__ words, uint64_t pos_base, uint64_t win0,
                                                      uint64_t winlen, uint64_t *__restrict__ d_start, uint64_t *__restrict__ d_end) {
    __shared__ uint32_t sW[3 * kGWaves];
    __shared__ uint32_t sN[kGWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint64_t group_base = words[kGwGroupBase];
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t cnt = tile_count[tile];
        const uint64_t r0 = group_base + tile_base[tile];
        if (cnt == 0 || r0 + cnt <= win0 || r0 >= win0 + winlen) continue;   // (the whole workgroup)
        uint32_t first = hit_bits[(uint64_t)tile * kGThreads + t];
        const uint32_t dl = delim_bits[(uint64_t)tile * kGThreads + t];
        const uint64_t tile1 = pos_base + (uint64_t)tile * kGTile + 1;
        const LaneCtx c = lane_ctx(0, dl, tile1, tile_ctx + kGCtx * (uint64_t)tile, sW);
        const uint32_t n = __popc(first);
        uint32_t inc = n;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            if (lane >= (uint32_t)o) inc += u;
        }
        if (lane == 63) sN[wv] = inc;   // (lane_ctx synchronised behind the readers of the tile before)
        __syncthreads();
        uint64_t rank = r0 + inc - n;
        for (uint32_t q = 0; q < wv; q++) rank += sN[q];
        const uint64_t base1 = tile1 + kGPer * t;
        while (first) {
            const uint32_t b = (uint32_t)__builtin_ctz(first);
            first &= first - 1;
            if (rank >= win0 && rank - win0 < winlen) {
                const uint32_t front = dl & ((1u << b) - 1);
                d_start[rank - win0] = front ? base1 + 31u - (uint32_t)__builtin_clz(front) : c.ld;
                const uint64_t end = end_behind(dl, b, base1, c.nd);
                if (end) d_end[rank - win0] = end;
            }
            rank++;
        }
    }
}

// the run's end: a line still open and selected ends at `total`
__global__ void k_gfinish(uint64_t *__restrict__ words, uint64_t total, uint64_t *__restrict__ d_end, uint64_t cap) {
    if (!words[kGwOpen]) return;
    const uint64_t slot = words[kGwLines] - 1;
    if (slot < cap) d_end[slot] = total;
    words[kGwBytes] += total - words[kGwLast];
    words[kGwOpen] = 0;
}

// the last `keep` (<= kFCarry) bytes of [src, src + len) to the end of the carry buffer
__global__ __launch_bounds__(kGThreads) void k_gcarry(const uint8_t *__restrict__ src, uint64_t len, uint32_t keep,
                                                      uint8_t *__restrict__ carry) {
    const uint32_t t = threadIdx.x;
    if (t < keep) carry[kFCarry - keep + t] = src[len - keep + t];
}

namespace {
const char *kGStageNames[] = {"index", "decode", "scan", "select", "summary"};
constexpr int kGStages = 5;

int ready(fcx_dctx *c) {
    GrepScratch &G = c->gp;
    if (!G.host_words) {
        FCX_TRY(G.words.reserve(8 * kGwWords, "grep words"));
        FCX_TRY(G.pat.reserve(kFCarry, "grep pattern"));
        FCX_TRY(G.carry.reserve(kFCarry, "grep carry"));
        FCX_HIP(G.host_words.alloc(8 * kGwWords));
    }
    return FCX_OK;
}
}  // namespace

int grep_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim, const uint8_t *pattern,
             uint32_t m, const GrepSink &sink, GrepCarry *carry, uint64_t *stats, hipStream_t st, uint64_t rec_base) {
    const bool fresh = !carry || carry->base == 0;   // (nothing was seen before a run at offset 0)
    if (fresh) {
        for (int i = 0; i < FCX_GREP_STATS; i++) stats[i] = 0;
        c->gp.scratch_bytes = 0;
    }
    if (nblocks == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    GrepScratch &G = c->gp;
    VerifyScratch &V = c->vf;
    const uint64_t window = c->fd.window ? c->fd.window : kGWindow;
    if (sink.on_line) {
        FCX_TRY(G.win_start.reserve(8 * window, "grep lines"));
        FCX_TRY(G.win_end.reserve(8 * window, "grep lines"));
    }
    RunTimes T(c, kGStages, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    uint8_t padded[kFCarry] = {};
    memcpy(padded, pattern, m);
    FCX_HIP(hipMemcpyAsync(G.pat, padded, kFCarry, hipMemcpyHostToDevice, st));
    if (fresh) {
        FCX_HIP(hipMemsetAsync(G.words, 0, 8 * kGwWords, st));
        G.carry_len = 0;
    }
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host, `padded` may go)
    const std::vector<uint64_t> &doff = ix.doff;
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups, nullptr, kFCarry));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most + kFCarry > kGMaxRange)
        return fail(FCX_ERR_ARG, "fcx_grep_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    const uint64_t tiles_most = (most + kFCarry + kGTile - 1) / kGTile;
    FCX_TRY(G.hit_bits.reserve(2ull * kGThreads * tiles_most, "grep hit bits"));
    FCX_TRY(G.delim_bits.reserve(2ull * kGThreads * tiles_most, "grep delimiter bits"));
    FCX_TRY(G.tile_sum.reserve(4ull * kGSum * tiles_most, "grep tile words"));
    FCX_TRY(G.tile_ctx.reserve(8ull * kGCtx * tiles_most, "grep tile words"));
    FCX_TRY(G.tile_count.reserve(4 * tiles_most, "grep tile words"));
    FCX_TRY(G.tile_base.reserve(4 * tiles_most, "grep tile words"));
    G.scratch_bytes = tiles_most * (4ull * kGThreads + 4 * kGSum + 8 * kGCtx + 8);
    const uint64_t base = carry ? carry->base : 0, total = base + doff[nblocks];
    std::vector<uint64_t> host_lines;
    uint8_t *const dec = V.buf + kFCarry;
    for (const RunGroup &g : groups) {
        const uint32_t cl = G.carry_len;
        if (cl) FCX_HIP(hipMemcpyAsync(dec - cl, G.carry + (kFCarry - cl), cl, hipMemcpyDeviceToDevice, st));
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, dec, g.gbytes, st, rec_base, "fcx_grep_shard"));
        T.mark(2);
        const uint8_t *src = dec - cl;
        const uint64_t len = cl + g.gbytes, njudged = len >= m ? len - m + 1 : 0;
        // a range shorter than the pattern judges nothing and is all carry: the next group sees its delimiters
        const uint32_t ntiles = njudged ? (uint32_t)((len + kGTile - 1) / kGTile) : 0;
        const uint32_t grid = std::min(ntiles, kGMaxGrid);
        const uint64_t pos_base = base + doff[g.g0] - cl;
        if (ntiles)
            hipLaunchKernelGGL(k_gscan, dim3(grid), dim3(kGThreads), 0, st, src, len, njudged, m, (uint32_t)delim, (const uint32_t *)G.pat,
                               ntiles, (uint16_t *)G.hit_bits, (uint16_t *)G.delim_bits, (uint32_t *)G.tile_sum, (uint64_t *)G.words);
        T.mark(3);
        if (ntiles) {
            hipLaunchKernelGGL(k_gtiles, dim3(1), dim3(kGBaseThreads), 0, st, (const uint32_t *)G.tile_sum, ntiles, pos_base,
                               (uint64_t *)G.tile_ctx, (uint64_t *)G.words, sink.d_end, sink.cap);
            hipLaunchKernelGGL(k_gmark, dim3(grid), dim3(kGThreads), 0, st, (uint16_t *)G.hit_bits, (const uint16_t *)G.delim_bits,
                               (const uint32_t *)G.tile_sum, (const uint64_t *)G.tile_ctx, ntiles, pos_base, (uint32_t *)G.tile_count,
                               (uint64_t *)G.words);
            hipLaunchKernelGGL(k_gbase, dim3(1), dim3(kGBaseThreads), 0, st, (const uint32_t *)G.tile_count, ntiles,
                               (uint32_t *)G.tile_base, (uint64_t *)G.words);
            if (sink.cap)
                hipLaunchKernelGGL(k_gwrite, dim3(grid), dim3(kGThreads), 0, st, (const uint16_t *)G.hit_bits,
                                   (const uint16_t *)G.delim_bits, (const uint64_t *)G.tile_ctx, (const uint32_t *)G.tile_count,
                                   (const uint32_t *)G.tile_base, ntiles, (const uint64_t *)G.words, pos_base, 0ull, sink.cap,
                                   sink.d_start, sink.d_end);
        }
        T.mark(4);
        FCX_HIP(hipGetLastError());
        FCX_TRY(T.add(1, 4));
        // what the next group needs of this one: source and destination are two buffers
        const uint32_t keep = (uint32_t)std::min<uint64_t>(m - 1, len);
        if (keep) hipLaunchKernelGGL(k_gcarry, dim3(1), dim3(kGThreads), 0, st, src, len, keep, (uint8_t *)G.carry);
        G.carry_len = keep;
        if (sink.on_line && carry && ntiles) {   // the group's lines, window after window of the same bitmaps
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
                hipLaunchKernelGGL(k_gwrite, dim3(grid), dim3(kGThreads), 0, st, (const uint16_t *)G.hit_bits,
                                   (const uint16_t *)G.delim_bits, (const uint64_t *)G.tile_ctx, (const uint32_t *)G.tile_count,
                                   (const uint32_t *)G.tile_base, ntiles, (const uint64_t *)G.words, pos_base, w0, n,
                                   (uint64_t *)G.win_start, (uint64_t *)G.win_end);
                FCX_HIP(hipGetLastError());
                host_lines.resize(2 * n);
                FCX_HIP(hipMemcpyAsync(host_lines.data(), G.win_start, 8 * n, hipMemcpyDeviceToHost, st));
                FCX_HIP(hipMemcpyAsync(host_lines.data() + n, G.win_end, 8 * n, hipMemcpyDeviceToHost, st));
                FCX_HIP(hipStreamSynchronize(st));
                for (uint64_t i = 0; i < n; i++) {
                    if (open && w0 + i + 1 == end) {   // the group's last line is still open: its end is to come
                        carry->held = true;
                        carry->held_start = host_lines[i];
                    } else {
                        sink.on_line(sink.user, host_lines[i], host_lines[n + i]);
                    }
                }
            }
        }
    }
    T.mark(4);
    if (!carry) hipLaunchKernelGGL(k_gfinish, dim3(1), dim3(1), 0, st, (uint64_t *)G.words, total, sink.d_end, sink.cap);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
    T.mark(5);
    FCX_HIP(hipStreamSynchronize(st));
    stats[0] = G.host_words[kGwLines];
    stats[1] = G.host_words[kGwBytes];
    stats[2] = G.host_words[kGwHits];
    stats[3] = G.host_words[kGwJudged];
    stats[4] = total;
    if (carry) carry->base = total;
    FCX_TRY(T.add(4, 5));
    T.publish(c, kGStageNames, kGStages);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_grep_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                   const uint8_t *pattern, uint32_t plen, uint64_t *d_start, uint64_t *d_end, uint64_t cap, uint64_t *stats,
                   void *stream) {
    if (!c || !pattern || !stats || (nblocks && !d_rec) || (cap && (!d_start || !d_end)))
        return fail(FCX_ERR_ARG, "fcx_grep_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_grep_shard: kind must be '7' or '8'");
    if (plen < 1 || plen > FCX_FIND_MAX_PATTERN) return fail(FCX_ERR_ARG, "fcx_grep_shard: pattern length outside [1, FCX_FIND_MAX_PATTERN]");
    if (memchr(pattern, delim, plen)) return fail(FCX_ERR_ARG, "fcx_grep_shard: the pattern holds the delimiter");
    GrepSink sink;
    sink.d_start = d_start;
    sink.d_end = d_end;
    sink.cap = cap;
    return grep_run(c, kind, d_rec, rec_len, nblocks, delim, pattern, plen, sink, nullptr, stats, (hipStream_t)stream, 0);
}

int fcx_dctx_grep_scratch(fcx_dctx *c, uint64_t *bytes) {
    if (!c || !bytes) return fail(FCX_ERR_ARG, "fcx_dctx_grep_scratch: NULL argument");
    *bytes = c->gp.scratch_bytes;
    return FCX_OK;
}

}  // extern "C"
