// fcx_context.hip — context and inverted grep on a device-resident run (gfx950): grep -v, -A, -B, -C as blocks of
// consecutive selected lines.  fcx_grep_blocks_shard of include/fcx.h (its stream and host forms: fcx_stream.hip,
// fcx_ranges.hip).  DESIGN.md §9k.
//
//   the run      grep_set_run's: index, then per record group the decode behind the carry, k_sscan<true> (the one
//                scan path, launched by fcx_set.hip) and k_gtiles, which leave the hit bits, the delimiter bits and
//                per tile the last delimiter and the last hit before it, over positions each seen exactly once.
//   k_cbase      a line's status is decided at the delimiter that ends it: it matches iff the last hit lies at or
//                behind its start.  One base bit per delimiter, and per tile its delimiters, its base lines and
//                the tile-local index of its first and last base line.
//   k_clines     one workgroup over those, seeded from the carried words: every tile gets its first line's number,
//                the last base line before it and the first base line behind it in the group.  Lane 0 then
//                resolves what the groups before left pending against the group's first base line h: the open
//                block's end (kXwPendEnd) stands iff h lies more than before + 1 lines behind it, and a block
//                starts at line max(h - before, 0) iff that line began in an earlier group and lies behind the
//                after-context of the last base line; its start comes from the ring.
//   k_cmark      everything else is line-number arithmetic at the delimiters.  With i the line a delimiter ends,
//                LB the last base line <= i and NB the first one > i: the delimiter ends a block iff i - LB ==
//                after and NB - i > before + 1, and a block starts behind it iff NB - i == before + 1 and i - LB >
//                after.  Where the group holds no NB the one candidate end goes to kXwPendEnd, and the starts of
//                the group's last before + 1 lines go to the ring (line number mod (before + 1)).
//   k_cscan      one workgroup: exclusive scans of the tiles' starts and ends.
//   k_cwrite     starts and ends to their ranks: the r-th start and the r-th end are block r.
//   k_cfinish    the run's end closes the open line (a base line or not), resolves against it, and ends the block
//                that is still open.
// Beside the grep's scratch: three bitmaps and 56 bytes per tile, the ring, 32 words.  Nothing grows with the hits,
// the lines or the blocks, and no byte of a line travels between groups.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_device.h"
#include "fcx_patset.h"

namespace fcx {

constexpr uint32_t kCThreads = 256;
constexpr uint32_t kCWaves = kCThreads / 64;
constexpr uint32_t kCPer = 16;                    // positions per lane
constexpr uint32_t kCTile = kCPer * kCThreads;    // positions per tile (4096): k_sscan's
constexpr uint32_t kCMaxGrid = 2048;
constexpr uint32_t kCBaseThreads = 1024;          // k_gtiles, k_clines and k_cscan: one workgroup of 1024
constexpr uint32_t kCNone = 0xFFFFFFFFu;
constexpr uint64_t kCNone64 = ~0ull;
constexpr uint32_t kCGSum = 4, kCGCtx = 3;        // words per tile of the grep's tile_sum / tile_ctx
constexpr uint32_t kCCs = 4, kCLctx = 3;          // words per tile of tile_cs / tile_lctx
constexpr uint32_t kCWindow = 1u << 20;           // blocks per window of the stream form by default
constexpr uint64_t kCMaxRange = 0xFFFF0000ull;    // bytes of [carry | group] at most

// exclusive prefix of v over the tile's 256 lanes (every thread calls it; sN: kCWaves words)
__device__ inline uint32_t tile_xscan(uint32_t v, uint32_t *sN) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += u;
    }
    __syncthreads();   // sN of the scan before is read
    if (lane == 63) sN[wv] = inc;
    __syncthreads();
    uint32_t pre = inc - v;
    for (uint32_t q = 0; q < wv; q++) pre += sN[q];
    return pre;
}

// block-wide exclusive maximum scan, forwards (blockDim.x threads, <= 16 waves); the maximum of all in *all
__device__ inline uint32_t cx_xmax(uint32_t v, uint32_t *sh, uint32_t *all) {
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

// block-wide exclusive minimum scan, backwards: the minimum over the threads behind this one (kCNone: none)
__device__ inline uint32_t cx_xmin_back(uint32_t v, uint32_t *sh, uint32_t *all) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_down(inc, o, 64);
        if (lane + (uint32_t)o < 64) inc = min(inc, u);
    }
    if (lane == 0) sh[wv] = inc;
    uint32_t suf = __shfl_down(inc, 1, 64);
    if (lane == 63) suf = kCNone;
    __syncthreads();
    uint32_t a = kCNone;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t x = sh[w];
        if (w > wv) suf = min(suf, x);
        a = min(a, x);
    }
    __syncthreads();
    *all = a;
    return suf;
}

// base_bits: bit b of a lane's word says that its delimiter bit b ends a base line (the line matches, or with
// `invert` does not).  tile_cs[4 k ..] = the tile's delimiters, its base lines, the index among its delimiters of
// the first one that ends a base line (kCNone: none) and 1 + that of the last (0: none).  hit_bits, delim_bits and
// tile_sum are k_sscan<true>'s, gctx k_gtiles' tile_ctx.
__global__ __launch_bounds__(kCThreads) void k_cbase(const uint16_t *__restrict__ hit_bits, const uint16_t *__restrict__ delim_bits,
                                                     const uint32_t *__restrict__ tile_sum, const uint64_t *__restrict__ gctx,
                                                     uint32_t ntiles, uint64_t pos_base, uint32_t invert,
                                                     uint16_t *__restrict__ base_bits, uint32_t *__restrict__ tile_cs) {
    __shared__ uint32_t sW[2 * kCWaves];
    __shared__ uint32_t sN[kCWaves];
    __shared__ uint32_t sR[4 * kCWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tile_sum[kCGSum * tile + 2] == 0) {   // (the whole workgroup) no delimiter: no line ends here
            if (t == 0) {
                tile_cs[kCCs * tile] = 0;
                tile_cs[kCCs * tile + 1] = 0;
                tile_cs[kCCs * tile + 2] = kCNone;
                tile_cs[kCCs * tile + 3] = 0;
            }
            continue;
        }
        const uint32_t h = hit_bits[(uint64_t)tile * kCThreads + t], dl = delim_bits[(uint64_t)tile * kCThreads + t];
        const uint64_t tile1 = pos_base + (uint64_t)tile * kCTile + 1;
        // the last delimiter and the last hit in front of the lane's positions, as 1 + position in the tile
        const uint32_t v_ld = dl ? kCPer * t + 32u - (uint32_t)__builtin_clz(dl) : 0u;
        const uint32_t v_lh = h ? kCPer * t + 32u - (uint32_t)__builtin_clz(h) : 0u;
        const uint64_t md = __ballot(dl != 0), mh = __ballot(h != 0), below = (1ull << lane) - 1;
        uint32_t ld = __shfl(v_ld, (md & below) ? 63 - __builtin_clzll(md & below) : 0, 64);
        uint32_t lh = __shfl(v_lh, (mh & below) ? 63 - __builtin_clzll(mh & below) : 0, 64);
        if (!(md & below)) ld = 0;
        if (!(mh & below)) lh = 0;
        const uint32_t w_ld = __shfl(v_ld, md ? 63 - __builtin_clzll(md) : 0, 64);
        const uint32_t w_lh = __shfl(v_lh, mh ? 63 - __builtin_clzll(mh) : 0, 64);
        __syncthreads();   // sW and sR of the tile before are read
        if (lane == 0) {
            sW[2 * wv] = md ? w_ld : 0u;
            sW[2 * wv + 1] = mh ? w_lh : 0u;
        }
        __syncthreads();
        for (uint32_t q = 0; q < wv; q++) {
            ld = max(ld, sW[2 * q]);
            lh = max(lh, sW[2 * q + 1]);
        }
        uint64_t cur = ld ? tile1 - 1 + ld : gctx[kCGCtx * (uint64_t)tile];       // the open line's start
        uint64_t ph = lh ? tile1 - 1 + lh : gctx[kCGCtx * (uint64_t)tile + 1];    // 1 + the last hit
        const uint64_t base1 = tile1 + kCPer * t;
        uint32_t u = h | dl, bs = 0;
        while (u) {
            const uint32_t b = (uint32_t)__builtin_ctz(u);
            u &= u - 1;
            if ((dl >> b) & 1) {
                if ((ph > cur) != (invert != 0)) bs |= 1u << b;
                cur = base1 + b;
            } else {
                ph = base1 + b;
            }
        }
        base_bits[(uint64_t)tile * kCThreads + t] = (uint16_t)bs;
        const uint32_t pre = tile_xscan(__popc(dl), sN);
        uint32_t nd = __popc(dl), nb = __popc(bs);
        uint32_t fb = bs ? pre + __popc(dl & ((1u << __builtin_ctz(bs)) - 1)) : kCNone;
        uint32_t lb = bs ? pre + __popc(dl & ((2u << (31 - __builtin_clz(bs))) - 1)) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nd += __shfl_xor(nd, o, 64);
            nb += __shfl_xor(nb, o, 64);
            fb = min(fb, (uint32_t)__shfl_xor(fb, o, 64));
            lb = max(lb, (uint32_t)__shfl_xor(lb, o, 64));
        }
        if (lane == 0) {
            sR[4 * wv] = nd;
            sR[4 * wv + 1] = nb;
            sR[4 * wv + 2] = fb;
            sR[4 * wv + 3] = lb;
        }
        __syncthreads();
        if (t == 0) {
            uint32_t a = 0, b = 0, f = kCNone, l = 0;
            for (uint32_t q = 0; q < kCWaves; q++) {
                a += sR[4 * q];
                b += sR[4 * q + 1];
                f = min(f, sR[4 * q + 2]);
                l = max(l, sR[4 * q + 3]);
            }
            tile_cs[kCCs * tile] = a;
            tile_cs[kCCs * tile + 1] = b;
            tile_cs[kCCs * tile + 2] = f;
            tile_cs[kCCs * tile + 3] = l;
        }
    }
}

// one block end or start more (a single thread): to its rank below cap, into the sums, and to the three words at
// `slot` for the stream forms
__device__ inline void cx_emit_end(uint64_t *w, const CxOut &o, uint64_t pos, uint64_t line, uint32_t slot) {
    const uint64_t r = w[kXwEnds];
    if (r < o.cap) o.d_end[r] = pos;
    w[kXwEnds] = r + 1;
    w[kXwSumEnd] += pos;
    w[kXwSumELine] += line + 1;
    w[slot] = 1;
    w[slot + 1] = pos;
    w[slot + 2] = line;
}
__device__ inline void cx_emit_start(uint64_t *w, const CxOut &o, uint64_t pos, uint64_t line) {
    const uint64_t r = w[kXwStarts];
    if (r < o.cap) {
        o.d_start[r] = pos;
        o.d_line[r] = line;
    }
    w[kXwStarts] = r + 1;
    w[kXwSumStart] += pos;
    w[kXwSumSLine] += line;
    w[kXwResStart] = 1;
    w[kXwResStart + 1] = pos;
    w[kXwResStart + 2] = line;
}

// Base line h arrives, the first behind kXwLastBase, with n0 lines closed in front of its group (a single thread).
// The pending end stands iff h does not reach it; the block of h starts at line j0 = max(h - before, 0) unless j0
// lies in or right behind the after-context of the last base line (one block then), and it starts here iff line j0
// began in front of the group: its start is in the ring (line 0 starts at 0).
__device__ inline void cx_resolve(uint64_t *w, const uint64_t *ring, uint32_t before, uint32_t after, uint64_t h, uint64_t n0,
                                  const CxOut &o) {
    const uint64_t lb1 = w[kXwLastBase];
    if (w[kXwPendEnd]) {
        const uint64_t pl = w[kXwPendLine];
        if (h - pl > (uint64_t)before + 1) cx_emit_end(w, o, w[kXwPendEnd], pl, kXwResEnd);
        w[kXwPendEnd] = 0;
    }
    const uint64_t j0 = h > before ? h - before : 0;
    if (j0 <= n0 && (lb1 == 0 || j0 > lb1 + after)) cx_emit_start(w, o, j0 ? ring[j0 % (before + 1)] : 0ull, j0);
}

// One workgroup.  tile_lctx[3 k ..] = the number of the line tile k's first delimiter ends, 1 + the last base line
// before the tile (0: none; reaches back through kXwLastBase), the first base line that ends behind the tile in
// this group (kCNone64: none).  Then the pending end and start are resolved against the group's first base line
// and the words advance: kXwLines, kXwLastBase, kXwBase, kXwGroupS / kXwGroupE.
__global__ __launch_bounds__(kCBaseThreads) void k_clines(const uint32_t *__restrict__ tile_cs, uint32_t ntiles, uint32_t before,
                                                          uint32_t after, uint64_t *__restrict__ tile_lctx,
                                                          uint64_t *__restrict__ words, const uint64_t *__restrict__ ring, CxOut out) {
    __shared__ uint32_t sh[kCBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (ntiles + kCBaseThreads - 1) / kCBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    const uint64_t n0 = words[kXwLines], lb0 = words[kXwLastBase];
    uint32_t s = 0, b = 0, tot_d, tot_b;
    for (uint32_t k = k0; k < k1; k++) {
        s += tile_cs[kCCs * k];
        b += tile_cs[kCCs * k + 1];
    }
    const uint32_t pre = block_xscan(s, sh, &tot_d);
    (void)block_xscan(b, sh, &tot_b);
    // this thread's tiles: 1 + the group-wide index of their last base delimiter, and the index of their first
    uint32_t a_lb = 0, a_fb = kCNone, run = pre;
    for (uint32_t k = k0; k < k1; k++) {
        const uint32_t fb = tile_cs[kCCs * k + 2], lb = tile_cs[kCCs * k + 3];
        if (lb) a_lb = run + lb;
        if (fb != kCNone && a_fb == kCNone) a_fb = run + fb;
        run += tile_cs[kCCs * k];
    }
    uint32_t g_lb, g_fb;
    uint32_t cur = cx_xmax(a_lb, sh, &g_lb);
    uint32_t nx = cx_xmin_back(a_fb, sh, &g_fb);
    run = pre;
    for (uint32_t k = k0; k < k1; k++) {
        tile_lctx[kCLctx * k] = n0 + run;
        tile_lctx[kCLctx * k + 1] = cur ? n0 + cur : lb0;
        if (tile_cs[kCCs * k + 3]) cur = run + tile_cs[kCCs * k + 3];
        run += tile_cs[kCCs * k];
    }
    for (uint32_t k = k1; k > k0; k--) {
        run -= tile_cs[kCCs * (k - 1)];
        tile_lctx[kCLctx * (k - 1) + 2] = nx != kCNone ? n0 + nx : kCNone64;
        const uint32_t fb = tile_cs[kCCs * (k - 1) + 2];
        if (fb != kCNone) nx = run + fb;
    }
    if (t == 0) {   // (every thread has read the words: the scans synchronised)
        words[kXwResEnd] = 0;
        words[kXwResStart] = 0;
        words[kXwFinEnd] = 0;
        if (g_fb != kCNone) cx_resolve(words, ring, before, after, n0 + g_fb, n0, out);
        words[kXwLines] = n0 + tot_d;
        if (g_lb) words[kXwLastBase] = n0 + g_lb;
        words[kXwBase] += tot_b;
        words[kXwGroupS] = words[kXwStarts];
        words[kXwGroupE] = words[kXwEnds];
    }
}

// Per tile: start_bits and end_bits (see the head of the file), tile_cnt[2 k ..] = the tile's starts and ends; the
// sums of the words advance; the candidate end without a base line behind it goes to kXwPendEnd / kXwPendLine
// (one delimiter of a group at most), the starts of the group's last before + 1 lines to the ring.
__global__ __launch_bounds__(kCThreads) void k_cmark(const uint16_t *__restrict__ delim_bits, const uint16_t *__restrict__ base_bits,
                                                     const uint32_t *__restrict__ tile_cs, const uint64_t *__restrict__ tile_lctx,
                                                     uint32_t ntiles, uint64_t pos_base, uint32_t before, uint32_t after,
                                                     uint16_t *__restrict__ start_bits, uint16_t *__restrict__ end_bits,
                                                     uint32_t *__restrict__ tile_cnt, uint64_t *__restrict__ words,
                                                     uint64_t *__restrict__ ring) {
    __shared__ uint32_t sN[kCWaves];
    __shared__ uint32_t sW[2 * kCWaves];
    __shared__ uint32_t sC[2 * kCWaves];
    __shared__ uint64_t sS[4 * kCWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint64_t n_end = words[kXwLines];   // (k_clines: the lines closed at the group's end)
    uint64_t sum_s = 0, sum_e = 0, sum_sl = 0, sum_el = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tile_cs[kCCs * tile] == 0) {   // (the whole workgroup) no delimiter
            if (t == 0) {
                tile_cnt[2 * tile] = 0;
                tile_cnt[2 * tile + 1] = 0;
            }
            continue;
        }
        const uint32_t dl = delim_bits[(uint64_t)tile * kCThreads + t], bs = base_bits[(uint64_t)tile * kCThreads + t];
        const uint32_t pre = tile_xscan(__popc(dl), sN);
        // tile-local: 1 + the index of the lane's last base delimiter, the index of its first
        const uint32_t v_lb = bs ? pre + __popc(dl & ((2u << (31 - __builtin_clz(bs))) - 1)) : 0u;
        const uint32_t v_fb = bs ? pre + __popc(dl & ((1u << __builtin_ctz(bs)) - 1)) : 0u;
        const uint64_t mb = __ballot(bs != 0), below = (1ull << lane) - 1, above = ~((2ull << lane) - 1);
        uint32_t lb = __shfl(v_lb, (mb & below) ? 63 - __builtin_clzll(mb & below) : 0, 64);
        uint32_t fb = __shfl(v_fb, (mb & above) ? __builtin_ctzll(mb & above) : 0, 64);
        if (!(mb & below)) lb = 0;
        bool has_nb = (mb & above) != 0;
        const uint32_t w_lb = __shfl(v_lb, mb ? 63 - __builtin_clzll(mb) : 0, 64);
        const uint32_t w_fb = __shfl(v_fb, mb ? __builtin_ctzll(mb) : 0, 64);
        __syncthreads();   // sW and sC of the tile before are read
        if (lane == 0) {
            sW[2 * wv] = mb ? w_lb : 0u;
            sW[2 * wv + 1] = mb ? w_fb : kCNone;
        }
        __syncthreads();
        for (uint32_t q = 0; q < wv; q++) lb = max(lb, sW[2 * q]);
        for (uint32_t q = wv + 1; q < kCWaves; q++)
            if (!has_nb && sW[2 * q + 1] != kCNone) {
                fb = sW[2 * q + 1];
                has_nb = true;
            }
        const uint64_t *lc = tile_lctx + kCLctx * (uint64_t)tile;
        const uint64_t line0 = lc[0];
        uint64_t lb1 = lb ? line0 + lb : lc[1];                 // 1 + the last base line so far
        const uint64_t nb_out = has_nb ? line0 + fb : lc[2];    // the first base line behind the lane
        const uint64_t base1 = pos_base + (uint64_t)tile * kCTile + 1 + kCPer * t;
        uint64_t i = line0 + pre;
        uint32_t u = dl, sb = 0, eb = 0;
        while (u) {
            const uint32_t b = (uint32_t)__builtin_ctz(u);
            u &= u - 1;
            const uint32_t behind = ~((2u << b) - 1);
            if ((bs >> b) & 1) lb1 = i + 1;
            const uint32_t rest = bs & behind;
            const uint64_t nb = rest ? i + __popc(dl & behind & ((2u << __builtin_ctz(rest)) - 1)) : nb_out;
            const bool far = lb1 == 0 || i + 1 - lb1 > after;   // line i lies behind the last base line's after-context
            const uint64_t e = base1 + b;                       // the line's end: the next line's start
            if (lb1 && i + 1 - lb1 == after) {
                if (nb == kCNone64) {
                    words[kXwPendEnd] = e;
                    words[kXwPendLine] = i;
                } else if (nb - i > (uint64_t)before + 1) {
                    eb |= 1u << b;
                    sum_e += e;
                    sum_el += i + 1;
                }
            }
            if (nb != kCNone64 && nb - i == (uint64_t)before + 1 && far) {
                sb |= 1u << b;
                sum_s += e;
                sum_sl += i + 1;
            }
            if (i + 1 + before >= n_end) ring[(i + 1) % (before + 1)] = e;
            i++;
        }
        start_bits[(uint64_t)tile * kCThreads + t] = (uint16_t)sb;
        end_bits[(uint64_t)tile * kCThreads + t] = (uint16_t)eb;
        uint32_t n = __popc(sb) | (uint32_t)__popc(eb) << 16;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) sC[wv] = n;
        __syncthreads();
        if (t == 0) {
            const uint32_t a = sC[0] + sC[1] + sC[2] + sC[3];
            tile_cnt[2 * tile] = a & 0xFFFFu;
            tile_cnt[2 * tile + 1] = a >> 16;
        }
    }
    sum_s = wave_sum_u64(sum_s);
    sum_e = wave_sum_u64(sum_e);
    sum_sl = wave_sum_u64(sum_sl);
    sum_el = wave_sum_u64(sum_el);
    if (lane == 0) {
        sS[4 * wv] = sum_s;
        sS[4 * wv + 1] = sum_e;
        sS[4 * wv + 2] = sum_sl;
        sS[4 * wv + 3] = sum_el;
    }
    __syncthreads();
    if (t < 4) {
        const uint64_t v = sS[t] + sS[4 + t] + sS[8 + t] + sS[12 + t];
        const uint32_t word = t == 0 ? kXwSumStart : t == 1 ? kXwSumEnd : t == 2 ? kXwSumSLine : kXwSumELine;
        if (v) atomicAdd((unsigned long long *)words + word, (unsigned long long)v);
    }
}

// One workgroup: tile_rank[2 k ..] = the starts and the ends of the group's tiles before k; kXwStarts / kXwEnds
// advance by the group's, which go to kXwGroupNS / kXwGroupNE.
__global__ __launch_bounds__(kCBaseThreads) void k_cscan(const uint32_t *__restrict__ tile_cnt, uint32_t ntiles,
                                                         uint32_t *__restrict__ tile_rank, uint64_t *__restrict__ words) {
    __shared__ uint32_t sh[kCBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (ntiles + kCBaseThreads - 1) / kCBaseThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    uint32_t s = 0, e = 0, tot_s, tot_e;
    for (uint32_t k = k0; k < k1; k++) {
        s += tile_cnt[2 * k];
        e += tile_cnt[2 * k + 1];
    }
    uint32_t rs = block_xscan(s, sh, &tot_s), re = block_xscan(e, sh, &tot_e);
    for (uint32_t k = k0; k < k1; k++) {
        tile_rank[2 * k] = rs;
        tile_rank[2 * k + 1] = re;
        rs += tile_cnt[2 * k];
        re += tile_cnt[2 * k + 1];
    }
    if (t == 0) {
        words[kXwStarts] += tot_s;
        words[kXwEnds] += tot_e;
        words[kXwGroupNS] = tot_s;
        words[kXwGroupNE] = tot_e;
    }
}

// The group's starts whose rank lies in [win_s, win_s + winlen) to o_start / o_line[rank - win_s], its ends whose
// rank lies in [win_e, win_e + winlen) to o_end / o_eline (may be null) likewise.  Ranks count from the call's
// blocks before the group's own (kXwGroupS / kXwGroupE), with `local` from 0.
__global__ __launch_bounds__(kCThreads) void k_cwrite(const uint16_t *__restrict__ delim_bits, const uint16_t *__restrict__ start_bits,
                                                      const uint16_t *__restrict__ end_bits, const uint32_t *__restrict__ tile_cnt,
                                                      const uint32_t *__restrict__ tile_rank, const uint64_t *__restrict__ tile_lctx,
                                                      uint32_t ntiles, const uint64_t *__restrict__ words, uint64_t pos_base,
                                                      uint32_t local, uint64_t win_s, uint64_t win_e, uint64_t winlen,
                                                      uint64_t *__restrict__ o_start, uint64_t *__restrict__ o_line,
                                                      uint64_t *__restrict__ o_end, uint64_t *__restrict__ o_eline) {
    __shared__ uint32_t sN[kCWaves];
    const uint32_t t = threadIdx.x;
    const uint64_t g_s = local ? 0ull : words[kXwGroupS], g_e = local ? 0ull : words[kXwGroupE];
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t cs = tile_cnt[2 * tile], ce = tile_cnt[2 * tile + 1];
        const uint64_t r0s = g_s + tile_rank[2 * tile], r0e = g_e + tile_rank[2 * tile + 1];
        const bool in_s = cs && r0s + cs > win_s && r0s < win_s + winlen, in_e = ce && r0e + ce > win_e && r0e < win_e + winlen;
        if (!in_s && !in_e) continue;   // (the whole workgroup)
        const uint32_t dl = delim_bits[(uint64_t)tile * kCThreads + t];
        const uint32_t sb = start_bits[(uint64_t)tile * kCThreads + t], eb = end_bits[(uint64_t)tile * kCThreads + t];
        const uint32_t pre_d = tile_xscan(__popc(dl), sN);
        const uint32_t pre_se = tile_xscan(__popc(sb) | (uint32_t)__popc(eb) << 16, sN);
        uint64_t rs = r0s + (pre_se & 0xFFFFu), re = r0e + (pre_se >> 16);
        const uint64_t line0 = tile_lctx[kCLctx * (uint64_t)tile] + pre_d;
        const uint64_t base1 = pos_base + (uint64_t)tile * kCTile + 1 + kCPer * t;
        uint32_t u = sb | eb;
        while (u) {
            const uint32_t b = (uint32_t)__builtin_ctz(u);
            u &= u - 1;
            const uint64_t i = line0 + __popc(dl & ((1u << b) - 1));   // the line the delimiter ends
            if ((sb >> b) & 1) {
                if (rs >= win_s && rs - win_s < winlen) {
                    o_start[rs - win_s] = base1 + b;
                    o_line[rs - win_s] = i + 1;
                }
                rs++;
            } else {
                if (re >= win_e && re - win_e < winlen) {
                    o_end[re - win_e] = base1 + b;
                    if (o_eline) o_eline[re - win_e] = i;
                }
                re++;
            }
        }
    }
}

// The run's end at `total`: the open line, if it has a byte, is a line like any other and closes here; a base line
// resolves what is pending; the block still open ends at the pending end or with the run's last line.
__global__ void k_cfinish(uint64_t *__restrict__ words, const uint64_t *__restrict__ gwords, const uint64_t *__restrict__ ring,
                          uint32_t before, uint32_t after, uint32_t invert, uint64_t total, CxOut out) {
    words[kXwResEnd] = 0;
    words[kXwResStart] = 0;
    words[kXwFinEnd] = 0;
    const uint64_t n = words[kXwLines], last = gwords[kGwLast];
    uint64_t nlines = n;
    if (total > last) {
        if ((gwords[kGwLastHit] > last) != (invert != 0)) {
            cx_resolve(words, ring, before, after, n, n, out);
            words[kXwLastBase] = n + 1;
            words[kXwBase] += 1;
        }
        nlines = n + 1;
    }
    if (words[kXwStarts] > words[kXwEnds]) {
        if (words[kXwPendEnd]) cx_emit_end(words, out, words[kXwPendEnd], words[kXwPendLine], kXwFinEnd);
        else cx_emit_end(words, out, total, nlines - 1, kXwFinEnd);
    }
    words[kXwPendEnd] = 0;
    words[kXwTotal] = nlines;
}

namespace {
const char *kCStageNames[] = {"index", "decode", "scan", "select", "summary"};
constexpr int kCStages = 5;
}  // namespace

int ready_context(fcx_dctx *c) {
    ContextScratch &C = c->cx;
    if (!C.host_words) {
        FCX_TRY(C.words.reserve(8 * kXwWords, "context words"));
        FCX_TRY(C.ring.reserve(8 * kCRing, "context ring"));
        FCX_HIP(C.host_words.alloc(8 * kXwWords));
    }
    return FCX_OK;
}

int reserve_context_tiles(fcx_dctx *c, uint64_t range_bytes) {
    ContextScratch &C = c->cx;
    GrepScratch &G = c->gp;
    const uint64_t tiles = (range_bytes + kCTile - 1) / kCTile + 1;
    G.scratch_bytes = C.grep_bytes;   // (the grep's part alone, so that its maximum stays its own)
    FCX_TRY(context_reserve(c, range_bytes));
    C.grep_bytes = G.scratch_bytes;
    FCX_TRY(C.base_bits.reserve(2ull * kCThreads * tiles, "context base bits"));
    FCX_TRY(C.start_bits.reserve(2ull * kCThreads * tiles, "context start bits"));
    FCX_TRY(C.end_bits.reserve(2ull * kCThreads * tiles, "context end bits"));
    FCX_TRY(C.tile_cs.reserve(4ull * kCCs * tiles, "context tile words"));
    FCX_TRY(C.tile_lctx.reserve(8ull * kCLctx * tiles, "context tile words"));
    FCX_TRY(C.tile_cnt.reserve(8 * tiles, "context tile words"));
    FCX_TRY(C.tile_rank.reserve(8 * tiles, "context tile words"));
    C.extra_bytes = std::max<uint64_t>(C.extra_bytes, tiles * (6ull * kCThreads + 4 * kCCs + 8 * kCLctx + 16) + 8ull * kCRing + 8ull * kXwWords);
    G.scratch_bytes = C.grep_bytes + C.extra_bytes;
    return FCX_OK;
}

CxOut out_of(const BlockSink &sink) { return CxOut{sink.d_start, sink.d_end, sink.d_line, sink.cap}; }

// the block that is open on the host side of the stream form gets its end, or a new one opens
void host_close(const BlockSink &sink, BlockCarry *carry, uint64_t end, uint64_t eline) {
    if (carry->held) sink.on_block(sink.user, carry->held_start, end, carry->held_line, eline - carry->held_line + 1);
    carry->held = false;
}
void host_open(BlockCarry *carry, uint64_t start, uint64_t line) {
    carry->held = true;
    carry->held_start = start;
    carry->held_line = line;
}
// what lane 0 of k_clines or k_cfinish resolved, in its order: the pending end, the pending start, the last end
void host_resolved(const BlockSink &sink, BlockCarry *carry, const uint64_t *hw) {
    if (hw[kXwResEnd]) host_close(sink, carry, hw[kXwResEnd + 1], hw[kXwResEnd + 2]);
    if (hw[kXwResStart]) host_open(carry, hw[kXwResStart + 1], hw[kXwResStart + 2]);
    if (hw[kXwFinEnd]) host_close(sink, carry, hw[kXwFinEnd + 1], hw[kXwFinEnd + 2]);
}

namespace {
// One range of a blocks call: scan, the select kernels, the first cap blocks or the windows of the stream form with
// the open block held back; the carry for the range behind it.
int blocks_scan(fcx_dctx *c, const fcx_pattern_set *set, uint8_t delim, const fcx_grep_opts &opts, const uint8_t *src, uint64_t len,
                bool final, uint64_t pos_base, const BlockSink &sink, BlockCarry *carry, uint64_t window,
                std::vector<uint64_t> *host_win, RunTimes *T, hipStream_t st) {
    GrepScratch &G = c->gp;
    ContextScratch &C = c->cx;
    const uint32_t invert = opts.flags & FCX_GREP_INVERT;
    uint32_t ntiles = 0;
    FCX_TRY(context_scan(c, set, delim, src, len, final, &ntiles, st));
    const uint32_t grid = std::min(ntiles, kCMaxGrid);
    if (T) T->mark(3);
    if (ntiles) {
        hipLaunchKernelGGL(k_gtiles, dim3(1), dim3(kCBaseThreads), 0, st, (const uint32_t *)G.tile_sum, ntiles, pos_base,
                           (uint64_t *)G.tile_ctx, (uint64_t *)G.words, (uint64_t *)nullptr, 0ull);
        hipLaunchKernelGGL(k_cbase, dim3(grid), dim3(kCThreads), 0, st, (const uint16_t *)G.hit_bits, (const uint16_t *)G.delim_bits,
                           (const uint32_t *)G.tile_sum, (const uint64_t *)G.tile_ctx, ntiles, pos_base, invert, (uint16_t *)C.base_bits,
                           (uint32_t *)C.tile_cs);
        hipLaunchKernelGGL(k_clines, dim3(1), dim3(kCBaseThreads), 0, st, (const uint32_t *)C.tile_cs, ntiles, opts.before, opts.after,
                           (uint64_t *)C.tile_lctx, (uint64_t *)C.words, (const uint64_t *)C.ring, out_of(sink));
        hipLaunchKernelGGL(k_cmark, dim3(grid), dim3(kCThreads), 0, st, (const uint16_t *)G.delim_bits, (const uint16_t *)C.base_bits,
                           (const uint32_t *)C.tile_cs, (const uint64_t *)C.tile_lctx, ntiles, pos_base, opts.before, opts.after,
                           (uint16_t *)C.start_bits, (uint16_t *)C.end_bits, (uint32_t *)C.tile_cnt, (uint64_t *)C.words,
                           (uint64_t *)C.ring);
        hipLaunchKernelGGL(k_cscan, dim3(1), dim3(kCBaseThreads), 0, st, (const uint32_t *)C.tile_cnt, ntiles, (uint32_t *)C.tile_rank,
                           (uint64_t *)C.words);
        if (sink.cap)
            hipLaunchKernelGGL(k_cwrite, dim3(grid), dim3(kCThreads), 0, st, (const uint16_t *)G.delim_bits,
                               (const uint16_t *)C.start_bits, (const uint16_t *)C.end_bits, (const uint32_t *)C.tile_cnt,
                               (const uint32_t *)C.tile_rank, (const uint64_t *)C.tile_lctx, ntiles, (const uint64_t *)C.words, pos_base,
                               0u, 0ull, 0ull, sink.cap, sink.d_start, sink.d_line, sink.d_end, (uint64_t *)nullptr);
    }
    if (T) T->mark(4);
    FCX_HIP(hipGetLastError());
    if (T) FCX_TRY(T->add(1, 4));
    const uint32_t keep = final ? 0u : (uint32_t)std::min<uint64_t>(set->max_len - 1, len);
    if (keep) hipLaunchKernelGGL(k_gcarry, dim3(1), dim3(kCThreads), 0, st, src, len, keep, (uint8_t *)G.carry);
    G.carry_len = keep;
    if (sink.on_block && carry && ntiles) {   // the range's blocks, window after window of the same bitmaps
        FCX_HIP(hipMemcpyAsync(C.host_words, C.words, 8 * kXwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        host_resolved(sink, carry, C.host_words);
        const uint64_t ns = C.host_words[kXwGroupNS], ne = C.host_words[kXwGroupNE];
        const bool end_first = carry->held;   // the group's own ends and starts alternate, an end first iff a block is open
        for (uint64_t w0 = 0; w0 < std::max(ns, ne); w0 += window) {
            const uint64_t cs = ns > w0 ? std::min(window, ns - w0) : 0, ce = ne > w0 ? std::min(window, ne - w0) : 0;
            hipLaunchKernelGGL(k_cwrite, dim3(grid), dim3(kCThreads), 0, st, (const uint16_t *)G.delim_bits,
                               (const uint16_t *)C.start_bits, (const uint16_t *)C.end_bits, (const uint32_t *)C.tile_cnt,
                               (const uint32_t *)C.tile_rank, (const uint64_t *)C.tile_lctx, ntiles, (const uint64_t *)C.words, pos_base,
                               1u, w0, w0, window, (uint64_t *)C.win[0], (uint64_t *)C.win[1], (uint64_t *)C.win[2],
                               (uint64_t *)C.win[3]);
            FCX_HIP(hipGetLastError());
            host_win->resize(2 * cs + 2 * ce);
            uint64_t *hs = host_win->data(), *hl = hs + cs, *he = hl + cs, *hel = he + ce;
            if (cs) {
                FCX_HIP(hipMemcpyAsync(hs, C.win[0], 8 * cs, hipMemcpyDeviceToHost, st));
                FCX_HIP(hipMemcpyAsync(hl, C.win[1], 8 * cs, hipMemcpyDeviceToHost, st));
            }
            if (ce) {
                FCX_HIP(hipMemcpyAsync(he, C.win[2], 8 * ce, hipMemcpyDeviceToHost, st));
                FCX_HIP(hipMemcpyAsync(hel, C.win[3], 8 * ce, hipMemcpyDeviceToHost, st));
            }
            FCX_HIP(hipStreamSynchronize(st));
            for (uint64_t i = 0; i < std::max(cs, ce); i++) {
                if (end_first && i < ce) host_close(sink, carry, he[i], hel[i]);
                if (i < cs) host_open(carry, hs[i], hl[i]);
                if (!end_first && i < ce) host_close(sink, carry, he[i], hel[i]);
            }
        }
    }
    return FCX_OK;
}
}  // namespace

// the eight stats from the words (the caller has synchronised)
void blocks_stats_out(fcx_dctx *c, uint64_t total, uint64_t *stats) {
    const uint64_t *w = c->cx.host_words, *g = c->gp.host_words;
    stats[0] = w[kXwStarts];
    stats[1] = w[kXwSumELine] - w[kXwSumSLine];
    stats[2] = w[kXwSumEnd] - w[kXwSumStart];
    stats[3] = w[kXwBase];
    stats[4] = g[kGwHits];
    stats[5] = g[kGwJudged];
    stats[6] = total;
    stats[7] = w[kXwTotal];
}

namespace {
// the run's end on the device, and the words to the host
int blocks_finish(fcx_dctx *c, const fcx_grep_opts &opts, const BlockSink &sink, uint64_t total, hipStream_t st) {
    GrepScratch &G = c->gp;
    ContextScratch &C = c->cx;
    hipLaunchKernelGGL(k_cfinish, dim3(1), dim3(1), 0, st, (uint64_t *)C.words, (const uint64_t *)G.words, (const uint64_t *)C.ring,
                       opts.before, opts.after, opts.flags & FCX_GREP_INVERT, total, out_of(sink));
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(C.host_words, C.words, 8 * kXwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
    return context_fetch(c, st);
}
}  // namespace

int blocks_args(const char *fn, const fcx_pattern_set *set, uint8_t delim, const fcx_grep_opts *opts) {
    FCX_TRY(set_args(fn, set, delim));
    if (!opts) return fail(FCX_ERR_ARG, std::string(fn) + ": NULL options");
    if (opts->flags & ~FCX_GREP_INVERT) return fail(FCX_ERR_ARG, std::string(fn) + ": unknown flag bits");
    if (opts->before > FCX_GREP_MAX_CONTEXT || opts->after > FCX_GREP_MAX_CONTEXT)
        return fail(FCX_ERR_ARG, std::string(fn) + ": context above FCX_GREP_MAX_CONTEXT");
    return FCX_OK;
}

int blocks_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
               const fcx_pattern_set *set, const fcx_grep_opts &opts, const BlockSink &sink, BlockCarry *carry, uint64_t *stats,
               uint64_t *counts, hipStream_t st, uint64_t rec_base) {
    const bool fresh = !carry || carry->base == 0;   // (nothing was seen before a run at offset 0)
    ContextScratch &C = c->cx;
    if (fresh) {
        for (int i = 0; i < FCX_GREP_BLOCK_STATS; i++) stats[i] = 0;
        c->gp.scratch_bytes = 0;
        C.grep_bytes = C.extra_bytes = 0;
        for (uint64_t &v : c->ps.stats) v = 0;
        for (uint32_t k = 0; k < set->npat && counts; k++) counts[k] = 0;
    }
    if (nblocks == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(context_ready(c, set, fresh, st));
    FCX_TRY(ready_context(c));
    GrepScratch &G = c->gp;
    VerifyScratch &V = c->vf;
    const uint64_t window = c->fd.window ? c->fd.window : kCWindow;
    if (sink.on_block)
        for (DevBuf<uint64_t> &w : C.win) FCX_TRY(w.reserve(8 * window, "context blocks"));
    RunTimes T(c, kCStages, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    if (fresh) {
        FCX_HIP(hipMemsetAsync(G.words, 0, 8 * kGwWords, st));
        FCX_HIP(hipMemsetAsync(C.words, 0, 8 * kXwWords, st));
        G.carry_len = 0;
    }
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host)
    const std::vector<uint64_t> &doff = ix.doff;
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups, nullptr, kFCarry));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most + kFCarry > kCMaxRange)
        return fail(FCX_ERR_ARG, "fcx_grep_blocks_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    FCX_TRY(reserve_context_tiles(c, most + kFCarry));
    const uint64_t base = carry ? carry->base : 0, total = base + doff[nblocks];
    std::vector<uint64_t> host_win;
    uint8_t *const dec = V.buf + kFCarry;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const RunGroup &g = groups[gi];
        const uint32_t cl = G.carry_len;
        if (cl) FCX_HIP(hipMemcpyAsync(dec - cl, G.carry + (kFCarry - cl), cl, hipMemcpyDeviceToDevice, st));
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, dec, g.gbytes, st, rec_base, "fcx_grep_blocks_shard"));
        T.mark(2);
        FCX_TRY(blocks_scan(c, set, delim, opts, dec - cl, cl + g.gbytes, !carry && gi + 1 == groups.size(), base + doff[g.g0] - cl, sink,
                            carry, window, &host_win, &T, st));
    }
    T.mark(4);
    if (!carry) {
        FCX_TRY(blocks_finish(c, opts, sink, total, st));
    } else {
        FCX_HIP(hipMemcpyAsync(C.host_words, C.words, 8 * kXwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
        FCX_TRY(context_fetch(c, st));
    }
    T.mark(5);
    FCX_HIP(hipStreamSynchronize(st));
    context_publish(c, set, counts);
    blocks_stats_out(c, total, stats);
    if (carry) carry->base = total;
    FCX_TRY(T.add(4, 5));
    T.publish(c, kCStageNames, kCStages);
    return FCX_OK;
}

int blocks_final(fcx_dctx *c, uint8_t delim, const fcx_pattern_set *set, const fcx_grep_opts &opts, const BlockSink &sink,
                 BlockCarry *carry, uint64_t *stats, uint64_t *counts, hipStream_t st) {
    GrepScratch &G = c->gp;
    ContextScratch &C = c->cx;
    if (carry->base == 0) {   // nothing was decoded: no line, no block; the end is a final pass all the same
        c->ps.stats[5]++;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    const uint32_t cl = G.carry_len;
    if (cl) {   // the positions the last group carried, each pattern bounded by the end
        const uint64_t window = c->fd.window ? c->fd.window : kCWindow;
        FCX_TRY(reserve_context_tiles(c, kFCarry));
        std::vector<uint64_t> host_win;
        FCX_TRY(blocks_scan(c, set, delim, opts, (const uint8_t *)G.carry + (kFCarry - cl), cl, true, carry->base - cl, sink, carry, window,
                            &host_win, nullptr, st));
    } else {
        c->ps.stats[5]++;
    }
    FCX_TRY(blocks_finish(c, opts, sink, carry->base, st));
    FCX_HIP(hipStreamSynchronize(st));
    if (sink.on_block) host_resolved(sink, carry, C.host_words);
    context_publish(c, set, counts);
    blocks_stats_out(c, carry->base, stats);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_grep_blocks_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                          const fcx_pattern_set *set, const fcx_grep_opts *opts, uint64_t *d_start, uint64_t *d_end, uint64_t *d_line,
                          uint64_t cap, uint64_t *stats, uint64_t *counts, void *stream) {
    if (!c || !set || !stats || (nblocks && !d_rec) || (cap && (!d_start || !d_end || !d_line)))
        return fail(FCX_ERR_ARG, "fcx_grep_blocks_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_grep_blocks_shard: kind must be '7' or '8'");
    FCX_TRY(blocks_args("fcx_grep_blocks_shard", set, delim, opts));
    BlockSink sink;
    sink.d_start = d_start;
    sink.d_end = d_end;
    sink.d_line = d_line;
    sink.cap = cap;
    return blocks_run(c, kind, d_rec, rec_len, nblocks, delim, set, *opts, sink, nullptr, stats, counts, (hipStream_t)stream, 0);
}

}  // extern "C"
