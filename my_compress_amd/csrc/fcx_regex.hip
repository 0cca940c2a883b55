// fcx_regex.hip — regular-expression grep on a device-resident run (gfx950): which lines of what the records decode
// to hold a match of a POSIX ERE, with -v, -A, -B, -C as blocks.  fcx_regex_*, fcx_grep_regex_blocks_shard of
// include/fcx.h (its stream and host forms: fcx_stream.hip, fcx_ranges.hip).  DESIGN.md §9l.
//
//   the run      blocks_run's (fcx_context.hip): index, then per record group the decode behind the carry, the scan,
//                k_gtiles and the select stage, all but the scan unchanged.  `$` looks one byte ahead, so this is the
//                set path with M = 2: a group that is not the run's last contributes all positions but its last
//                byte, which it carries together with the DFA state in front of it (a device word).
//   the scan     a DFA is sequential in its state, and the delimiter that resets it may lie any number of tiles back.
//                Three launches over k_sscan's tiles (256 lanes, 16 positions each) compose state maps:
//   k_rmap       every lane runs all S states through its 16 bytes (S chains of next[cls[b]][state] in LDS, eight at
//                a time), the 256 lane maps are composed in LDS, the tile's map S -> S goes out, S bytes.
//   k_rentry     one workgroup: every thread composes the maps of a stretch of tiles, the threads' maps are composed
//                from the group's entry state, the stretch is walked again with that one state: the state in front
//                of every tile, and the group's exit state for the next group.
//   k_rmark      lane maps again, from the tile's entry state every lane's entry state, then the one real chain:
//                hit bit p where the state is in acc, or in acc_eol with d or the run's end behind p; delimiter bits
//                and tile summary as k_sscan<true> writes them.
// No workgroup waits for another: the three launches order the work.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"
#include "fcx_regex.h"

namespace fcx {

constexpr uint32_t kRThreads = 256;
constexpr uint32_t kRWaves = kRThreads / 64;
constexpr uint32_t kRPer = 16;                          // positions per lane
constexpr uint32_t kRTile = kRPer * kRThreads;          // positions per tile (4096): k_sscan's
constexpr uint32_t kRMaxGrid = 2048;
constexpr uint32_t kRBaseThreads = 1024;                // k_gtiles, k_clines and k_cscan: one workgroup of 1024
constexpr uint32_t kRNone = 0xFFFFFFFFu;
constexpr uint32_t kRSum = 4;                           // words per tile of the grep's tile_sum
constexpr uint32_t kRWindow = 1u << 20;                 // blocks per window of the stream form by default
constexpr uint64_t kRMaxRange = 0xFFFF0000ull;          // bytes of [carry | group] at most
constexpr uint32_t kRMapStride = kRxMaxStride;          // bytes of a lane's map in LDS: 17 dwords, so lanes spread over the banks
constexpr uint32_t kRSegs = 16, kRSegLanes = kRThreads / kRSegs;
constexpr uint32_t kRMaxS = FCX_REGEX_MAX_STATES;
constexpr uint32_t kRKeep = 1;                          // bytes a group carries: `$` looks one byte ahead
static_assert(kRMaxS % 8 == 0 && kRMaxS <= kRMapStride, "lane maps: eight states at a time");

// bit q of the result: byte q of the dword equals the byte replicated in rep (the carry-free zero-byte form)
__device__ inline uint32_t rx_eq_bits4(uint32_t x, uint32_t rep) {
    x ^= rep;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

struct RxLds {
    __attribute__((aligned(16))) uint8_t block[kRxBlockBytes];
    __attribute__((aligned(16))) uint8_t map[kRThreads * kRMapStride];   // the lanes' (k_rentry: the threads') maps
    uint8_t seg[kRSegs * kRMaxS];                                          // the maps of 16 lanes each, composed
    uint8_t seg_entry[kRSegs];
    uint8_t lane_entry[kRThreads];
};

__device__ inline void rx_stage(RxLds &L, const uint8_t *__restrict__ block, uint32_t block_bytes) {
    for (uint32_t j = threadIdx.x; j < block_bytes / 16; j += blockDim.x) ((uint4 *)L.block)[j] = ((const uint4 *)block)[j];
}

// the 16 bytes of piece (base + 16 t) of [src, src + len), zeros behind the range
__device__ inline uint4 rx_piece(const uint8_t *__restrict__ src, uint64_t i, uint32_t sh, uint64_t len) {
    uint4 w = make_uint4(0, 0, 0, 0);
    if (i + 16 <= len) {
        w = ld16_bounded(src, i, sh, len);
    } else if (i < len) {   // the range's last bytes
        uint32_t x[4] = {0, 0, 0, 0};
        for (uint32_t q = 0; q < (uint32_t)(len - i); q++) x[q >> 2] |= (uint32_t)src[i + q] << (8 * (q & 3));
        w = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return w;
}

// the rows of the transition table that the lane's 16 bytes select (byte offsets into the block)
__device__ inline void rx_rows(const RxLds &L, const uint4 &w, uint32_t stride, uint32_t (&rows)[kRPer]) {
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (uint32_t b = 0; b < kRPer; b++) rows[b] = kRxNext + (uint32_t)L.block[kRxCls + ((x[b >> 2] >> (8 * (b & 3))) & 0xFFu)] * stride;
}

// The map of the lane's first nb bytes, state -> state for the S states, to `out` (kRMapStride bytes): S independent
// chains, eight at a time in registers.  States from S on map like S - 1 (never read).
__device__ inline void rx_lane_map(const RxLds &L, const uint32_t (&rows)[kRPer], uint32_t nb, uint32_t S, uint8_t *out) {
    for (uint32_t s0 = 0; s0 < S; s0 += 8) {
        uint32_t st[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) st[i] = min(s0 + i, S - 1);
#pragma unroll
        for (uint32_t b = 0; b < kRPer; b++) {
            if (b < nb) {
#pragma unroll
                for (uint32_t i = 0; i < 8; i++) st[i] = L.block[rows[b] + st[i]];
            }
        }
        ((uint32_t *)(out + s0))[0] = st[0] | st[1] << 8 | st[2] << 16 | st[3] << 24;
        ((uint32_t *)(out + s0))[1] = st[4] | st[5] << 8 | st[6] << 16 | st[7] << 24;
    }
}

// L.seg[seg][s] = where the 16 maps of segment seg, composed in order, take state s (256 threads; it synchronises)
__device__ inline void rx_seg_maps(RxLds &L, uint32_t S) {
    __syncthreads();   // the maps are written
    for (uint32_t idx = threadIdx.x; idx < kRSegs * kRMaxS; idx += kRThreads) {
        const uint32_t seg = idx / kRMaxS, s = idx % kRMaxS;
        if (s >= S) continue;
        uint32_t st = s;
        for (uint32_t l = seg * kRSegLanes; l < (seg + 1) * kRSegLanes; l++) st = L.map[l * kRMapStride + st];
        L.seg[seg * kRMaxS + s] = (uint8_t)st;
    }
    __syncthreads();
}

// From the state `entry` in front of map 0: L.lane_entry[l] = the state in front of map l, for the 256 maps whose
// segments rx_seg_maps composed.  It synchronises.
__device__ inline void rx_entries(RxLds &L, uint32_t entry) {
    if (threadIdx.x == 0) {
        uint32_t st = entry;
        for (uint32_t seg = 0; seg < kRSegs; seg++) {
            L.seg_entry[seg] = (uint8_t)st;
            st = L.seg[seg * kRMaxS + st];
        }
    }
    __syncthreads();
    if (threadIdx.x < kRSegs) {
        uint32_t st = L.seg_entry[threadIdx.x];
        for (uint32_t l = threadIdx.x * kRSegLanes; l < (threadIdx.x + 1) * kRSegLanes; l++) {
            L.lane_entry[l] = (uint8_t)st;
            st = L.map[l * kRMapStride + st];
        }
    }
    __syncthreads();
}

// tile_map[S k ..] = the map of the positions of tile k below njudged, for the ntiles tiles of [src, src + len)
__global__ __launch_bounds__(kRThreads) void k_rmap(const uint8_t *__restrict__ src, uint64_t len, uint64_t njudged,
                                                    const uint8_t *__restrict__ block, uint32_t block_bytes, uint32_t ntiles,
                                                    uint8_t *__restrict__ tile_map) {
    __shared__ RxLds L;
    const uint32_t t = threadIdx.x;
    rx_stage(L, block, block_bytes);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
    __syncthreads();
    const uint32_t *hd = (const uint32_t *)L.block;
    const uint32_t S = hd[kRxHStates], stride = hd[kRxHStride];
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t at = (uint64_t)tile * kRTile + kRPer * t;   // this lane's first position
        const uint32_t nb = at >= njudged ? 0u : (uint32_t)min((uint64_t)kRPer, njudged - at);
        const uint4 w = rx_piece(src, at, sh, len);
        uint32_t rows[kRPer];
        rx_rows(L, w, stride, rows);
        __syncthreads();   // the readers of the tile before are done
        rx_lane_map(L, rows, nb, S, L.map + t * kRMapStride);
        rx_seg_maps(L, S);
        if (t < S) {
            uint32_t st = t;
            for (uint32_t seg = 0; seg < kRSegs; seg++) st = L.seg[seg * kRMaxS + st];
            tile_map[(uint64_t)tile * S + t] = (uint8_t)st;
        }
    }
}

// the state a fresh run starts in
__global__ void k_rinit(uint32_t *__restrict__ state, uint32_t start) { state[0] = start; }

// One workgroup.  tile_entry[k] = the state in front of tile k, from state[0] in front of tile 0; state[0] = the
// state behind the last tile.
__global__ __launch_bounds__(kRThreads) void k_rentry(const uint8_t *__restrict__ tile_map, uint32_t ntiles, uint32_t S,
                                                      uint8_t *__restrict__ tile_entry, uint32_t *__restrict__ state) {
    __shared__ __attribute__((aligned(16))) uint8_t sMap[kRThreads * kRMapStride];
    __shared__ uint8_t sSeg[kRSegs * kRMaxS];
    __shared__ uint8_t sSegEntry[kRSegs];
    __shared__ uint8_t sEntry[kRThreads];
    const uint32_t t = threadIdx.x, per = (ntiles + kRThreads - 1) / kRThreads;
    const uint32_t k0 = min(t * per, ntiles), k1 = min(k0 + per, ntiles);
    for (uint32_t s0 = 0; s0 < S; s0 += 8) {   // the stretch's map, eight chains at a time
        uint32_t st[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) st[i] = min(s0 + i, S - 1);
        for (uint32_t k = k0; k < k1; k++) {
            const uint8_t *m = tile_map + (uint64_t)k * S;
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) st[i] = m[st[i]];
        }
        ((uint32_t *)(sMap + t * kRMapStride + s0))[0] = st[0] | st[1] << 8 | st[2] << 16 | st[3] << 24;
        ((uint32_t *)(sMap + t * kRMapStride + s0))[1] = st[4] | st[5] << 8 | st[6] << 16 | st[7] << 24;
    }
    __syncthreads();
    for (uint32_t idx = t; idx < kRSegs * kRMaxS; idx += kRThreads) {
        const uint32_t seg = idx / kRMaxS, s = idx % kRMaxS;
        if (s >= S) continue;
        uint32_t st = s;
        for (uint32_t l = seg * kRSegLanes; l < (seg + 1) * kRSegLanes; l++) st = sMap[l * kRMapStride + st];
        sSeg[seg * kRMaxS + s] = (uint8_t)st;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t st = state[0];
        for (uint32_t seg = 0; seg < kRSegs; seg++) {
            sSegEntry[seg] = (uint8_t)st;
            st = sSeg[seg * kRMaxS + st];
        }
        state[0] = st;   // behind every tile
    }
    __syncthreads();
    if (t < kRSegs) {
        uint32_t st = sSegEntry[t];
        for (uint32_t l = t * kRSegLanes; l < (t + 1) * kRSegLanes; l++) {
            sEntry[l] = (uint8_t)st;
            st = sMap[l * kRMapStride + st];
        }
    }
    __syncthreads();
    uint32_t st = sEntry[t];
    for (uint32_t k = k0; k < k1; k++) {   // the stretch again, with the one state
        tile_entry[k] = (uint8_t)st;
        st = tile_map[(uint64_t)k * S + st];
    }
}

// The positions [0, njudged) of [src, src + len): bit p & 15 of hit_bits[p >> 4] says whether a match ends at p (the
// byte behind p decides for acc_eol: the delimiter, or with p + 1 == len the run's end, which only a final range
// judges), delim_bits likewise for src[p] == delim, and tile_out[4 k ..] = the tile's hits, 1 + its first delimiter,
// 1 + its last delimiter, 1 + its last hit: k_sscan<true>'s outputs.  w_judged and w_hits advance.
__global__ __launch_bounds__(kRThreads) void k_rmark(const uint8_t *__restrict__ src, uint64_t len, uint64_t njudged,
                                                     const uint8_t *__restrict__ block, uint32_t block_bytes, uint32_t ntiles,
                                                     const uint8_t *__restrict__ tile_entry, uint16_t *__restrict__ hit_bits,
                                                     uint16_t *__restrict__ delim_bits, uint32_t *__restrict__ tile_out,
                                                     uint64_t *__restrict__ w_judged, uint64_t *__restrict__ w_hits) {
    __shared__ RxLds L;
    __shared__ uint32_t sR[4 * kRWaves];
    __shared__ uint64_t sJ[2 * kRWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    rx_stage(L, block, block_bytes);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
    __syncthreads();
    const uint32_t *hd = (const uint32_t *)L.block;
    const uint32_t S = hd[kRxHStates], stride = hd[kRxHStride], delim = hd[kRxHDelim], rep = delim * 0x01010101u;
    const uint64_t acc = (uint64_t)hd[kRxHAcc] | (uint64_t)hd[kRxHAcc + 1] << 32;
    const uint64_t acc_eol = (uint64_t)hd[kRxHAccEol] | (uint64_t)hd[kRxHAccEol + 1] << 32;
    uint64_t judged = 0, nhits = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t at = (uint64_t)tile * kRTile + kRPer * t;   // this lane's first position
        const uint32_t nb = at >= njudged ? 0u : (uint32_t)min((uint64_t)kRPer, njudged - at);
        const uint4 w = rx_piece(src, at, sh, len);
        uint32_t behind = __shfl_down(w.x, 1, 64) & 0xFFu;   // the byte behind the lane's 16
        if (lane == 63) behind = at + kRPer < len ? src[at + kRPer] : delim;
        uint32_t rows[kRPer];
        rx_rows(L, w, stride, rows);
        __syncthreads();   // the readers of the tile before are done
        rx_lane_map(L, rows, nb, S, L.map + t * kRMapStride);
        rx_seg_maps(L, S);
        rx_entries(L, tile_entry[tile]);
        uint32_t dl = rx_eq_bits4(w.x, rep) | rx_eq_bits4(w.y, rep) << 4 | rx_eq_bits4(w.z, rep) << 8 | rx_eq_bits4(w.w, rep) << 12;
        // the positions with the delimiter or the range's end behind them (bytes behind the range were loaded as zeros)
        uint32_t ends = dl >> 1 | (uint32_t)(behind == delim) << 15;
        if (at + kRPer >= len) ends |= at < len ? ~0u << (uint32_t)(len - 1 - at) : ~0u;
        dl &= (1u << nb) - 1;
        uint32_t st = L.lane_entry[t], hits = 0;
#pragma unroll
        for (uint32_t b = 0; b < kRPer; b++) {
            if (b < nb) {
                st = L.block[rows[b] + st];
                const uint32_t h = (uint32_t)(acc >> st) | ((uint32_t)(acc_eol >> st) & (ends >> b));
                hits |= (h & 1u) << b;
            }
        }
        hit_bits[(uint64_t)tile * kRThreads + t] = (uint16_t)hits;
        delim_bits[(uint64_t)tile * kRThreads + t] = (uint16_t)dl;
        judged += nb;
        // the tile's summary: positions in the range, 1 + position
        const uint32_t at1 = (uint32_t)at + 1;
        uint32_t n = __popc(hits);
        uint32_t fd = dl ? at1 + (uint32_t)__builtin_ctz(dl) : kRNone;
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
            uint32_t tn = 0, tf = kRNone, tl = 0, th = 0;
            for (uint32_t q = 0; q < kRWaves; q++) {
                tn += sR[4 * q];
                tf = min(tf, sR[4 * q + 1]);
                tl = max(tl, sR[4 * q + 2]);
                th = max(th, sR[4 * q + 3]);
            }
            tile_out[kRSum * tile] = tn;
            tile_out[kRSum * tile + 1] = tf == kRNone ? 0u : tf;
            tile_out[kRSum * tile + 2] = tl;
            tile_out[kRSum * tile + 3] = th;
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
        uint64_t j = 0, h = 0;
        for (uint32_t q = 0; q < kRWaves; q++) {
            j += sJ[2 * q];
            h += sJ[2 * q + 1];
        }
        if (j) atomicAdd((unsigned long long *)w_judged, (unsigned long long)j);
        if (h) atomicAdd((unsigned long long *)w_hits, (unsigned long long)h);
    }
}

namespace {
const char *kRStageNames[] = {"index", "decode", "scan", "select", "summary"};
constexpr int kRStages = 5;

// what the grep's own calls set up (either may come first), and the regex's block on the device
int ready_regex(fcx_dctx *c, const fcx_regex *re, bool fresh, hipStream_t st) {
    GrepScratch &G = c->gp;
    RegexScratch &R = c->rx;
    if (!G.host_words) {
        FCX_TRY(G.words.reserve(8 * kGwWords, "grep words"));
        FCX_TRY(G.pat.reserve(kFCarry, "grep pattern"));
        FCX_TRY(G.carry.reserve(kFCarry, "grep carry"));
        FCX_HIP(G.host_words.alloc(8 * kGwWords));
    }
    FCX_TRY(R.block.reserve(kRxBlockBytes, "regex"));
    FCX_TRY(R.state.reserve(16, "regex state"));
    FCX_HIP(hipMemcpyAsync(R.block, re->block, re->block_bytes, hipMemcpyHostToDevice, st));
    if (fresh) {
        hipLaunchKernelGGL(k_rinit, dim3(1), dim3(1), 0, st, (uint32_t *)R.state, re->start);
        FCX_HIP(hipGetLastError());
    }
    return FCX_OK;
}

int reserve_regex_tiles(fcx_dctx *c, const fcx_regex *re, uint64_t range_bytes) {
    RegexScratch &R = c->rx;
    const uint64_t tiles = (range_bytes + kRTile - 1) / kRTile + 1;
    FCX_TRY(reserve_context_tiles(c, range_bytes));
    FCX_TRY(R.tile_map.reserve((uint64_t)re->nstates * tiles, "regex tile maps"));
    FCX_TRY(R.tile_entry.reserve(tiles, "regex tile states"));
    R.tile_bytes = std::max<uint64_t>(R.tile_bytes, tiles * (re->nstates + 1ull));
    c->gp.scratch_bytes += R.tile_bytes;   // (reserve_context_tiles has set the grep's and the blocks calls' part)
    return FCX_OK;
}

// One range of a regex call: blocks_scan (fcx_context.hip) with the three scan launches in k_sscan<true>'s place and
// one carried byte.
int regex_scan(fcx_dctx *c, const fcx_regex *re, const fcx_grep_opts &opts, const uint8_t *src, uint64_t len, bool final,
               uint64_t pos_base, const BlockSink &sink, BlockCarry *carry, uint64_t window, std::vector<uint64_t> *host_win, RunTimes *T,
               hipStream_t st) {
    GrepScratch &G = c->gp;
    ContextScratch &C = c->cx;
    RegexScratch &R = c->rx;
    const uint32_t invert = opts.flags & FCX_GREP_INVERT;
    // hit bits and delimiter bits over the same positions, each seen by exactly one range: all of a final range, all
    // but the last byte otherwise
    const uint64_t njudged = final ? len : (len > kRKeep ? len - kRKeep : 0);
    const uint32_t ntiles = (uint32_t)((njudged + kRTile - 1) / kRTile);
    const uint32_t grid = std::min(ntiles, kRMaxGrid);
    if (ntiles) {
        hipLaunchKernelGGL(k_rmap, dim3(grid), dim3(kRThreads), 0, st, src, len, njudged, (const uint8_t *)R.block, re->block_bytes, ntiles,
                           (uint8_t *)R.tile_map);
        hipLaunchKernelGGL(k_rentry, dim3(1), dim3(kRThreads), 0, st, (const uint8_t *)R.tile_map, ntiles, re->nstates,
                           (uint8_t *)R.tile_entry, (uint32_t *)R.state);
        hipLaunchKernelGGL(k_rmark, dim3(grid), dim3(kRThreads), 0, st, src, len, njudged, (const uint8_t *)R.block, re->block_bytes,
                           ntiles, (const uint8_t *)R.tile_entry, (uint16_t *)G.hit_bits, (uint16_t *)G.delim_bits,
                           (uint32_t *)G.tile_sum, (uint64_t *)G.words + kGwJudged, (uint64_t *)G.words + kGwHits);
    }
    R.stats[2]++;
    if (final) R.stats[3]++;
    if (T) T->mark(3);
    if (ntiles) {
        hipLaunchKernelGGL(k_gtiles, dim3(1), dim3(kRBaseThreads), 0, st, (const uint32_t *)G.tile_sum, ntiles, pos_base,
                           (uint64_t *)G.tile_ctx, (uint64_t *)G.words, (uint64_t *)nullptr, 0ull);
        hipLaunchKernelGGL(k_cbase, dim3(grid), dim3(kRThreads), 0, st, (const uint16_t *)G.hit_bits, (const uint16_t *)G.delim_bits,
                           (const uint32_t *)G.tile_sum, (const uint64_t *)G.tile_ctx, ntiles, pos_base, invert, (uint16_t *)C.base_bits,
                           (uint32_t *)C.tile_cs);
        hipLaunchKernelGGL(k_clines, dim3(1), dim3(kRBaseThreads), 0, st, (const uint32_t *)C.tile_cs, ntiles, opts.before, opts.after,
                           (uint64_t *)C.tile_lctx, (uint64_t *)C.words, (const uint64_t *)C.ring, out_of(sink));
        hipLaunchKernelGGL(k_cmark, dim3(grid), dim3(kRThreads), 0, st, (const uint16_t *)G.delim_bits, (const uint16_t *)C.base_bits,
                           (const uint32_t *)C.tile_cs, (const uint64_t *)C.tile_lctx, ntiles, pos_base, opts.before, opts.after,
                           (uint16_t *)C.start_bits, (uint16_t *)C.end_bits, (uint32_t *)C.tile_cnt, (uint64_t *)C.words,
                           (uint64_t *)C.ring);
        hipLaunchKernelGGL(k_cscan, dim3(1), dim3(kRBaseThreads), 0, st, (const uint32_t *)C.tile_cnt, ntiles, (uint32_t *)C.tile_rank,
                           (uint64_t *)C.words);
        if (sink.cap)
            hipLaunchKernelGGL(k_cwrite, dim3(grid), dim3(kRThreads), 0, st, (const uint16_t *)G.delim_bits,
                               (const uint16_t *)C.start_bits, (const uint16_t *)C.end_bits, (const uint32_t *)C.tile_cnt,
                               (const uint32_t *)C.tile_rank, (const uint64_t *)C.tile_lctx, ntiles, (const uint64_t *)C.words, pos_base,
                               0u, 0ull, 0ull, sink.cap, sink.d_start, sink.d_line, sink.d_end, (uint64_t *)nullptr);
    }
    if (T) T->mark(4);
    FCX_HIP(hipGetLastError());
    if (T) FCX_TRY(T->add(1, 4));
    const uint32_t keep = final ? 0u : (uint32_t)std::min<uint64_t>(kRKeep, len);
    if (keep) hipLaunchKernelGGL(k_gcarry, dim3(1), dim3(kRThreads), 0, st, src, len, keep, (uint8_t *)G.carry);
    G.carry_len = keep;
    if (sink.on_block && carry && ntiles) {   // the range's blocks, window after window of the same bitmaps
        FCX_HIP(hipMemcpyAsync(C.host_words, C.words, 8 * kXwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        host_resolved(sink, carry, C.host_words);
        const uint64_t ns = C.host_words[kXwGroupNS], ne = C.host_words[kXwGroupNE];
        const bool end_first = carry->held;   // the group's own ends and starts alternate, an end first iff a block is open
        for (uint64_t w0 = 0; w0 < std::max(ns, ne); w0 += window) {
            const uint64_t cs = ns > w0 ? std::min(window, ns - w0) : 0, ce = ne > w0 ? std::min(window, ne - w0) : 0;
            hipLaunchKernelGGL(k_cwrite, dim3(grid), dim3(kRThreads), 0, st, (const uint16_t *)G.delim_bits,
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

// the run's end on the device, and the words to the host
int regex_finish(fcx_dctx *c, const fcx_grep_opts &opts, const BlockSink &sink, uint64_t total, hipStream_t st) {
    GrepScratch &G = c->gp;
    ContextScratch &C = c->cx;
    hipLaunchKernelGGL(k_cfinish, dim3(1), dim3(1), 0, st, (uint64_t *)C.words, (const uint64_t *)G.words, (const uint64_t *)C.ring,
                       opts.before, opts.after, opts.flags & FCX_GREP_INVERT, total, out_of(sink));
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(C.host_words, C.words, 8 * kXwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
    return FCX_OK;
}

void regex_publish(fcx_dctx *c) {
    c->rx.stats[0] = c->gp.host_words[kGwJudged];
    c->rx.stats[1] = c->gp.host_words[kGwHits];
}
}  // namespace

int regex_args(const char *fn, const fcx_regex *re, const fcx_grep_opts *opts) {
    if (!re || re->nstates < 1 || re->nstates > FCX_REGEX_MAX_STATES) return fail(FCX_ERR_ARG, std::string(fn) + ": not a regex");
    if (!opts) return fail(FCX_ERR_ARG, std::string(fn) + ": NULL options");
    if (opts->flags & ~FCX_GREP_INVERT) return fail(FCX_ERR_ARG, std::string(fn) + ": unknown flag bits");
    if (opts->before > FCX_GREP_MAX_CONTEXT || opts->after > FCX_GREP_MAX_CONTEXT)
        return fail(FCX_ERR_ARG, std::string(fn) + ": context above FCX_GREP_MAX_CONTEXT");
    return FCX_OK;
}

int regex_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_regex *re,
              const fcx_grep_opts &opts, const BlockSink &sink, BlockCarry *carry, uint64_t *stats, hipStream_t st, uint64_t rec_base) {
    const bool fresh = !carry || carry->base == 0;   // (nothing was seen before a run at offset 0)
    ContextScratch &C = c->cx;
    if (fresh) {
        for (int i = 0; i < FCX_GREP_BLOCK_STATS; i++) stats[i] = 0;
        c->gp.scratch_bytes = 0;
        C.grep_bytes = C.extra_bytes = 0;
        for (uint64_t &v : c->rx.stats) v = 0;
        c->rx.tile_bytes = 0;
    }
    if (nblocks == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready_regex(c, re, fresh, st));
    FCX_TRY(ready_context(c));
    GrepScratch &G = c->gp;
    VerifyScratch &V = c->vf;
    const uint64_t window = c->fd.window ? c->fd.window : kRWindow;
    if (sink.on_block)
        for (DevBuf<uint64_t> &w : C.win) FCX_TRY(w.reserve(8 * window, "context blocks"));
    RunTimes T(c, kRStages, st);
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
    if (most + kFCarry > kRMaxRange)
        return fail(FCX_ERR_ARG, "fcx_grep_regex_blocks_shard: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    FCX_TRY(reserve_regex_tiles(c, re, most + kFCarry));
    const uint64_t base = carry ? carry->base : 0, total = base + doff[nblocks];
    std::vector<uint64_t> host_win;
    uint8_t *const dec = V.buf + kFCarry;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const RunGroup &g = groups[gi];
        const uint32_t cl = G.carry_len;
        if (cl) FCX_HIP(hipMemcpyAsync(dec - cl, G.carry + (kFCarry - cl), cl, hipMemcpyDeviceToDevice, st));
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, dec, g.gbytes, st, rec_base,
                             "fcx_grep_regex_blocks_shard"));
        T.mark(2);
        FCX_TRY(regex_scan(c, re, opts, dec - cl, cl + g.gbytes, !carry && gi + 1 == groups.size(), base + doff[g.g0] - cl, sink, carry,
                           window, &host_win, &T, st));
    }
    T.mark(4);
    if (!carry) {
        FCX_TRY(regex_finish(c, opts, sink, total, st));
    } else {
        FCX_HIP(hipMemcpyAsync(C.host_words, C.words, 8 * kXwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipMemcpyAsync(G.host_words, G.words, 8 * kGwWords, hipMemcpyDeviceToHost, st));
    }
    T.mark(5);
    FCX_HIP(hipStreamSynchronize(st));
    regex_publish(c);
    blocks_stats_out(c, total, stats);
    if (carry) carry->base = total;
    FCX_TRY(T.add(4, 5));
    T.publish(c, kRStageNames, kRStages);
    return FCX_OK;
}

int regex_final(fcx_dctx *c, const fcx_regex *re, const fcx_grep_opts &opts, const BlockSink &sink, BlockCarry *carry, uint64_t *stats,
                hipStream_t st) {
    GrepScratch &G = c->gp;
    ContextScratch &C = c->cx;
    if (carry->base == 0) {   // nothing was decoded: no line, no block; the end is a final pass all the same
        c->rx.stats[3]++;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    const uint32_t cl = G.carry_len;
    if (cl) {   // the byte the last group carried, with the run's end behind it
        const uint64_t window = c->fd.window ? c->fd.window : kRWindow;
        FCX_TRY(reserve_regex_tiles(c, re, kFCarry));
        std::vector<uint64_t> host_win;
        FCX_TRY(regex_scan(c, re, opts, (const uint8_t *)G.carry + (kFCarry - cl), cl, true, carry->base - cl, sink, carry, window,
                           &host_win, nullptr, st));
    } else {
        c->rx.stats[3]++;
    }
    FCX_TRY(regex_finish(c, opts, sink, carry->base, st));
    FCX_HIP(hipStreamSynchronize(st));
    if (sink.on_block) host_resolved(sink, carry, C.host_words);
    regex_publish(c);
    blocks_stats_out(c, carry->base, stats);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_regex_create(fcx_regex **re, const uint8_t *expr, uint32_t len, uint8_t delim, uint32_t flags) {
    if (!re) return fail(FCX_ERR_ARG, "fcx_regex_create: NULL argument");
    *re = nullptr;
    fcx_regex *r = new (std::nothrow) fcx_regex();
    if (!r) return fail(FCX_ERR_NOMEM, "fcx_regex_create: out of memory");
    const std::string why = regex_compile(r, expr, len, delim, flags);
    if (!why.empty()) {
        delete r;
        return fail(FCX_ERR_ARG, "fcx_regex_create: " + why);
    }
    *re = r;
    return FCX_OK;
}

void fcx_regex_destroy(fcx_regex *re) { delete re; }

int fcx_regex_info(const fcx_regex *re, uint32_t *states, uint32_t *classes, uint32_t *flags, uint8_t *delim) {
    if (!re) return fail(FCX_ERR_ARG, "fcx_regex_info: NULL regex");
    if (states) *states = re->nstates;
    if (classes) *classes = re->nclasses;
    if (flags) *flags = re->flags;
    if (delim) *delim = re->delim;
    return FCX_OK;
}

int fcx_grep_regex_blocks_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_regex *re,
                                const fcx_grep_opts *opts, uint64_t *d_start, uint64_t *d_end, uint64_t *d_line, uint64_t cap,
                                uint64_t *stats, void *stream) {
    if (!c || !re || !stats || (nblocks && !d_rec) || (cap && (!d_start || !d_end || !d_line)))
        return fail(FCX_ERR_ARG, "fcx_grep_regex_blocks_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_grep_regex_blocks_shard: kind must be '7' or '8'");
    FCX_TRY(regex_args("fcx_grep_regex_blocks_shard", re, opts));
    BlockSink sink;
    sink.d_start = d_start;
    sink.d_end = d_end;
    sink.d_line = d_line;
    sink.cap = cap;
    return regex_run(c, kind, d_rec, rec_len, nblocks, re, *opts, sink, nullptr, stats, (hipStream_t)stream, 0);
}

int fcx_dctx_regex_scan_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_regex_scan_stats: bad argument");
    for (int i = 0; i < n && i < FCX_REGEX_SCAN_STATS; i++) out[i] = c->rx.stats[i];
    return FCX_OK;
}

}  // extern "C"
