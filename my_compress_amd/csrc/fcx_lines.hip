// fcx_lines.hip — line access on a device-resident run (gfx950): how many delimiter bytes do the records
// decode to, where does line j start, on which line does an offset lie?  fcx_lines_index_shard,
// fcx_lines_locate_shard, fcx_decompress_lines_shard and fcx_lines_of_shard of include/fcx.h (their stream
// and host forms: fcx_stream.hip).  DESIGN.md §9h.
//
//   the run      on the run core: index, then per record group the decode into the
//                verification's bounded buffer and the kernels below.  A delimiter is one byte, so no group
//                needs bytes of the one before it: what is carried is a number, the delimiters so far.
//   k_lcount     a wave per chunk of kLChunk = 4096 decoded bytes, grid-strided: each lane loads four 16-byte
//                pieces through ld16_bounded (nothing outside the range is read; the last piece byte by
//                byte), compares them with the delimiter replicated, counts per dword with the carry-free
//                zero-byte form and the wave sums: chunk_count[chunk].  No LDS tile, no bitmap.  Per
//                workgroup one atomic add of the bytes counted and one atomic maximum of the last delimiter.
//   k_lbase      one workgroup: the exclusive scan of the chunk counts, and the call's delimiters so far.
//   k_lrank      a thread per offset that lies in the group's decoded range: group base + chunk base + the
//                delimiters of the chunk in front of the offset, re-read by 16-byte pieces.  Over the group's
//                record boundaries this is the line index; over a caller's offsets it also checks their
//                order and bound.
//   k_lselect    the position of the r-th delimiter of the call, for two ranks: the wave whose chunk holds r
//                finds it by popcount and prefix.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"

namespace fcx {

constexpr uint32_t kLThreads = 256;
constexpr uint32_t kLWaves = kLThreads / 64;
constexpr uint32_t kLChunk = 4096;                 // decoded bytes per chunk: one wave, four pieces per lane
constexpr uint32_t kLRounds = kLChunk / (64 * 16);   // pieces per lane and chunk
constexpr uint32_t kLMaxGrid = 2048;               // workgroups of k_lcount / k_lselect / k_lrank at most
constexpr uint32_t kLBaseThreads = 1024;
constexpr uint64_t kLMaxGroup = 0xFFFF0000ull;     // bytes of a group at most (u32 counts)
constexpr uint64_t kLNone = ~0ull;

// bit 7 of every byte of x that is zero, and of no other: the carry-free form.  (The usual
// (x - 0x01010101) & ~x & 0x80808080 also flags a 0x01 byte above a zero byte: right for "any", wrong for a count.)
__device__ inline uint32_t zero_bytes(uint32_t x) {
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// The piece at byte i of [src, src + len) against the delimiter replicated: m[q] flags the equal bytes of dword
// q (bit 7 of each), bytes from len on never; returns the piece's bytes inside the range (0 .. 16).
__device__ inline uint32_t piece_flags(const uint8_t *__restrict__ src, uint64_t i, uint32_t sh, uint64_t len, uint32_t rep,
                                       uint32_t m[4]) {
    m[0] = m[1] = m[2] = m[3] = 0;
    if (i >= len) return 0;
    if (i + 16 <= len) {
        const uint4 w = ld16_bounded(src, i, sh, len);
        m[0] = zero_bytes(w.x ^ rep);
        m[1] = zero_bytes(w.y ^ rep);
        m[2] = zero_bytes(w.z ^ rep);
        m[3] = zero_bytes(w.w ^ rep);
        return 16;
    }
    const uint32_t nb = (uint32_t)(len - i);   // the range's last bytes
    const uint8_t d = (uint8_t)rep;
    for (uint32_t q = 0; q < nb; q++)
        if (src[i + q] == d) m[q >> 2] |= 0x80u << (8 * (q & 3));
    return nb;
}

// the 16 equal-byte flags of a piece as bits 0 .. 15, in byte order
__device__ inline uint32_t piece_bits(const uint32_t m[4]) {
    uint32_t b = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) b |= ((((m[q] >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * q);
    return b;
}

// chunk_count[k] = bytes equal to the delimiter in [src + k kLChunk, ...) of [src, src + len); words: kLwBytes
// advances by the bytes counted, kLwLast rises to pos_base + 1 + the position of the last delimiter.
__global__ __launch_bounds__(kLThreads) void k_lcount(const uint8_t *__restrict__ src, uint64_t len, uint32_t delim, uint32_t nchunks,
                                                     uint64_t pos_base, uint32_t *__restrict__ chunk_count,
                                                     uint64_t *__restrict__ words) {
    __shared__ uint64_t sB[kLWaves], sL[kLWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15), rep = delim * 0x01010101u;
    uint64_t bytes = 0, last = 0;
    for (uint32_t ch = blockIdx.x * kLWaves + wv; ch < nchunks; ch += gridDim.x * kLWaves) {
        const uint64_t base = (uint64_t)ch * kLChunk;
        uint32_t n = 0;
#pragma unroll
        for (uint32_t k = 0; k < kLRounds; k++) {
            const uint64_t i = base + 16ull * (64 * k + lane);
            uint32_t m[4];
            bytes += piece_flags(src, i, sh, len, rep, m);
            n += __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
                if (m[q]) last = max(last, i + 4 * q + ((31u - (uint32_t)__builtin_clz(m[q])) >> 3) + 1);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) chunk_count[ch] = n;
    }
    bytes = wave_sum_u64(bytes);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)last, o, 64), hi = __shfl_xor((uint32_t)(last >> 32), o, 64);
        last = max(last, ((uint64_t)hi << 32) | lo);
    }
    if (lane == 0) {
        sB[wv] = bytes;
        sL[wv] = last;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long *w = (unsigned long long *)words;
        uint64_t b = 0, l = 0;
        for (uint32_t q = 0; q < kLWaves; q++) {
            b += sB[q];
            l = max(l, sL[q]);
        }
        if (b) atomicAdd(w + kLwBytes, (unsigned long long)b);
        if (l) atomicMax(w + kLwLast, (unsigned long long)(pos_base + l));
    }
}

// One workgroup: chunk_base[k] = delimiters of the group's chunks before k; words: kLwGroupBase = the call's
// delimiters before this group, kLwTotal advanced by the group's.
__global__ __launch_bounds__(kLBaseThreads) void k_lbase(const uint32_t *__restrict__ chunk_count, uint32_t nchunks,
                                                         uint32_t *__restrict__ chunk_base, uint64_t *__restrict__ words) {
    __shared__ uint32_t sh[kLBaseThreads / 64];
    const uint32_t t = threadIdx.x, per = (nchunks + kLBaseThreads - 1) / kLBaseThreads;
    const uint32_t k0 = min(t * per, nchunks), k1 = min(k0 + per, nchunks);
    uint32_t s = 0, tot;
    for (uint32_t k = k0; k < k1; k++) s += chunk_count[k];
    uint32_t run = block_xscan(s, sh, &tot);
    for (uint32_t k = k0; k < k1; k++) {
        chunk_base[k] = run;
        run += chunk_count[k];
    }
    if (t == 0) {
        const uint64_t before = words[kLwTotal];
        words[kLwGroupBase] = before;
        words[kLwTotal] = before + tot;
    }
}

// out[i] = the delimiters in front of offs[i], for every i < noff whose offset lies in [g_lo, g_hi) of the
// group decoded at [src, src + len) (len = g_hi - g_lo), or is g_hi itself when incl_end.  With check (the
// offsets are a caller's) every thread also judges offs[i] <= bound and offs[i - 1] <= offs[i]: the first i
// that fails goes to kLwBadIndex by an atomic minimum.
__global__ __launch_bounds__(kLThreads) void k_lrank(const uint8_t *__restrict__ src, uint64_t len, uint32_t delim,
                                                    const uint32_t *__restrict__ chunk_base, uint64_t *__restrict__ words,
                                                    uint64_t g_lo, uint32_t incl_end, uint32_t check, uint64_t bound,
                                                    const uint64_t *__restrict__ offs, uint64_t noff, uint64_t *__restrict__ out) {
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15), rep = delim * 0x01010101u;
    const uint64_t group_base = words[kLwGroupBase], total = words[kLwTotal];
    for (uint64_t i = (uint64_t)blockIdx.x * kLThreads + threadIdx.x; i < noff; i += (uint64_t)gridDim.x * kLThreads) {
        const uint64_t x = offs[i];
        if (check && (x > bound || (i > 0 && offs[i - 1] > x))) {
            atomicMin((unsigned long long *)words + kLwBadIndex, (unsigned long long)i);
            continue;
        }
        if (x < g_lo || x - g_lo > len) continue;
        const uint64_t rel = x - g_lo;
        if (rel == len) {   // the group's end: every delimiter of the group lies in front of it
            if (incl_end) out[i] = total;
            continue;
        }
        const uint32_t ch = (uint32_t)(rel / kLChunk);
        uint64_t p = (uint64_t)ch * kLChunk;
        uint32_t n = 0;
        for (; p + 16 <= rel; p += 16) {
            uint32_t m[4];
            piece_flags(src, p, sh, len, rep, m);
            n += __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
        }
        for (; p < rel; p++) n += src[p] == (uint8_t)delim;
        out[i] = group_base + chunk_base[ch] + n;
    }
}

// words[kLwSel + q] = pos_base + 1 + the position in [src, src + len) of the r[q]-th delimiter of the call, for
// each of the two ranks the group holds (kLwGroupBase < r <= kLwTotal); the word of a rank it does not hold is
// left as it is.  A wave per chunk: the lanes' pieces in byte order, round by round.
__global__ __launch_bounds__(kLThreads) void k_lselect(const uint8_t *__restrict__ src, uint64_t len, uint32_t delim,
                                                      const uint32_t *__restrict__ chunk_count,
                                                      const uint32_t *__restrict__ chunk_base, uint32_t nchunks,
                                                      uint64_t *__restrict__ words, uint64_t pos_base, uint64_t r0, uint64_t r1) {
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15), rep = delim * 0x01010101u;
    const uint64_t group_base = words[kLwGroupBase];
    const uint64_t r[2] = {r0, r1};
    for (uint32_t ch = blockIdx.x * kLWaves + wv; ch < nchunks; ch += gridDim.x * kLWaves) {
        const uint64_t lo = group_base + chunk_base[ch];
        const uint32_t cnt = chunk_count[ch];
        for (uint32_t q = 0; q < 2; q++) {
            if (r[q] == kLNone || r[q] <= lo || r[q] - lo > cnt) continue;   // (the whole wave)
            uint32_t want = (uint32_t)(r[q] - lo);                           // the want-th of the chunk, 1-based
            for (uint32_t k = 0; k < kLRounds; k++) {
                const uint64_t i = (uint64_t)ch * kLChunk + 16ull * (64 * k + lane);
                uint32_t m[4];
                piece_flags(src, i, sh, len, rep, m);
                uint32_t bits = piece_bits(m);
                const uint32_t c = __popc(bits);
                uint32_t inc = c;
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t u = __shfl_up(inc, o, 64);
                    if (lane >= (uint32_t)o) inc += u;
                }
                const uint32_t all = __shfl(inc, 63, 64);
                if (want <= all) {
                    if (inc - c < want && want <= inc) {
                        for (uint32_t skip = want - (inc - c) - 1; skip; skip--) bits &= bits - 1;
                        words[kLwSel + q] = pos_base + i + (uint32_t)__builtin_ctz(bits) + 1;
                    }
                    break;
                }
                want -= all;
            }
        }
    }
}

namespace {
const char *kLStageNames[] = {"index", "decode", "count", "summary"};
constexpr int kLStages = 4;

int ready(fcx_dctx *c) {
    LinesScratch &S = c->ln;
    if (!S.host_words) {
        FCX_TRY(S.words.reserve(8 * kLwWords, "line words"));
        FCX_HIP(S.host_words.alloc(8 * kLwWords));
    }
    for (uint64_t &v : S.stats) v = 0;
    return FCX_OK;
}

uint32_t grid_for(uint64_t items, uint32_t per) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per - 1) / per, 1), kLMaxGrid); }

// the status words as a call starts: what the run continues from, the presets
void preset(uint64_t *w, const LinesReq &q) {
    for (uint32_t i = 0; i < kLwWords; i++) w[i] = 0;
    w[kLwTotal] = q.nl_before;
    w[kLwLast] = q.last_before;
    w[kLwBadIndex] = w[kLwSel] = w[kLwSel + 1] = kLNone;
}

// count and scan of the len bytes at src, which start at decoded offset pos (file-wide), on st
void launch_count(LinesScratch &S, const uint8_t *src, uint64_t len, uint8_t delim, uint64_t pos, hipStream_t st) {
    const uint32_t nchunks = (uint32_t)((len + kLChunk - 1) / kLChunk);
    if (nchunks)
        hipLaunchKernelGGL(k_lcount, dim3(grid_for(nchunks, kLWaves)), dim3(kLThreads), 0, st, src, len, (uint32_t)delim, nchunks, pos,
                           (uint32_t *)S.chunk_count, (uint64_t *)S.words);
    hipLaunchKernelGGL(k_lbase, dim3(1), dim3(kLBaseThreads), 0, st, (const uint32_t *)S.chunk_count, nchunks, (uint32_t *)S.chunk_base,
                       (uint64_t *)S.words);
}

void launch_select(LinesScratch &S, const uint8_t *src, uint64_t len, uint8_t delim, uint64_t pos, const uint64_t *sel, hipStream_t st) {
    const uint32_t nchunks = (uint32_t)((len + kLChunk - 1) / kLChunk);
    if (!nchunks) return;
    hipLaunchKernelGGL(k_lselect, dim3(grid_for(nchunks, kLWaves)), dim3(kLThreads), 0, st, src, len, (uint32_t)delim,
                       (const uint32_t *)S.chunk_count, (const uint32_t *)S.chunk_base, nchunks, (uint64_t *)S.words, pos, sel[0], sel[1]);
    S.stats[4]++;
}

int chunk_room(LinesScratch &S, uint64_t most) {
    const uint64_t chunks = (most + kLChunk - 1) / kLChunk;
    FCX_TRY(S.chunk_count.reserve(4 * chunks, "line chunk counts"));
    return S.chunk_base.reserve(4 * chunks, "line chunk counts");
}
}  // namespace

int lines_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, LinesReq &req, LinesRes *res,
              hipStream_t st, uint64_t rec_base) {
    *res = LinesRes();
    res->nl = req.nl_before;
    res->last = req.last_before;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    LinesScratch &S = c->ln;
    VerifyScratch &V = c->vf;
    RunTimes T(c, kLStages, st);
    RunIndex ix;
    if (nblocks) {
        FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
        FCX_TRY(T.add(0, 1));
    } else {
        ix.roff.assign(1, 0);
        ix.doff.assign(1, 0);
    }
    uint64_t w0[kLwWords];
    preset(w0, req);
    FCX_HIP(hipMemcpyAsync(S.words, w0, 8 * kLwWords, hipMemcpyHostToDevice, st));
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host, `w0` may go)
    const std::vector<uint64_t> &doff = ix.doff;
    res->decoded = doff[nblocks];
    if (req.staged) FCX_TRY(req.staged(res->decoded, &req));
    std::vector<RunGroup> groups;
    if (nblocks) FCX_TRY(run_groups(c, ix, nblocks, &groups));
    uint64_t most = 0;
    for (const RunGroup &g : groups) most = std::max(most, g.gbytes);
    if (most > kLMaxGroup) return fail(FCX_ERR_ARG, "fcx_lines: a record group of 4 GiB or more (fcx_dctx_set_verify_group)");
    FCX_TRY(chunk_room(S, most));
    const bool selecting = req.sel[0] != kLNone || req.sel[1] != kLNone;
    if (req.stop_early && !selecting) groups.clear();   // (nothing to look for: the index has answered)
    const uint64_t end = req.base + res->decoded;
    if (groups.empty() && req.noff) {   // a run without records: offsets of 0 lie at its end
        hipLaunchKernelGGL(k_lbase, dim3(1), dim3(kLBaseThreads), 0, st, (const uint32_t *)S.chunk_count, 0u, (uint32_t *)S.chunk_base,
                           (uint64_t *)S.words);
        hipLaunchKernelGGL(k_lrank, dim3(grid_for(req.noff, kLThreads)), dim3(kLThreads), 0, st, (const uint8_t *)V.buf, 0ull,
                           (uint32_t)req.delim, (const uint32_t *)S.chunk_base, (uint64_t *)S.words, req.base, req.last_run ? 1u : 0u,
                           req.check_offsets ? 1u : 0u, end, req.d_offsets, req.noff, req.d_lines);
        S.stats[3] += req.noff;
    }
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const RunGroup &g = groups[gi];
        const bool last_group = gi + 1 == groups.size();
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, g.g1 - g.g0, V.buf, g.gbytes, st, rec_base, "fcx_lines"));
        T.mark(2);
        const uint64_t g_lo = req.base + doff[g.g0];
        launch_count(S, V.buf, g.gbytes, req.delim, g_lo, st);
        if (req.d_line_off)   // the group's record boundaries; a boundary at the group's end has all of it in front
            hipLaunchKernelGGL(k_lrank, dim3(grid_for(g.g1 - g.g0 + 1, kLThreads)), dim3(kLThreads), 0, st, (const uint8_t *)V.buf, g.gbytes,
                               (uint32_t)req.delim, (const uint32_t *)S.chunk_base, (uint64_t *)S.words, doff[g.g0], 1u, 0u, 0ull,
                               (const uint64_t *)c->rg.dec_off + g.g0, (uint64_t)(g.g1 - g.g0 + 1), req.d_line_off + g.g0);
        if (req.noff)   // a thread per offset per group: the ones outside the group leave at once
            hipLaunchKernelGGL(k_lrank, dim3(grid_for(req.noff, kLThreads)), dim3(kLThreads), 0, st, (const uint8_t *)V.buf, g.gbytes,
                               (uint32_t)req.delim, (const uint32_t *)S.chunk_base, (uint64_t *)S.words, g_lo,
                               last_group && req.last_run ? 1u : 0u, req.check_offsets && gi == 0 ? 1u : 0u, end, req.d_offsets, req.noff,
                               req.d_lines);
        if (selecting) launch_select(S, V.buf, g.gbytes, req.delim, g_lo, req.sel, st);
        T.mark(3);
        FCX_HIP(hipGetLastError());
        FCX_TRY(T.add(1, 3));
        S.stats[1] += g.g1 - g.g0;
        S.stats[2]++;
        if (req.stop_early && !last_group) {   // is the answer complete?
            FCX_HIP(hipMemcpyAsync(S.host_words, S.words, 8 * kLwWords, hipMemcpyDeviceToHost, st));
            FCX_HIP(hipStreamSynchronize(st));
            bool open = false;
            for (int q = 0; q < 2; q++) open = open || (req.sel[q] != kLNone && S.host_words[kLwSel + q] == kLNone);
            if (!open) break;
        }
    }
    if (req.d_line_off) S.stats[3] += (uint64_t)nblocks + 1;
    if (req.noff && !groups.empty()) S.stats[3] += req.noff;
    T.mark(3);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(S.host_words, S.words, 8 * kLwWords, hipMemcpyDeviceToHost, st));
    T.mark(4);
    FCX_HIP(hipStreamSynchronize(st));
    const uint64_t *hw = S.host_words;
    S.stats[0] = hw[kLwBytes];
    res->nl = hw[kLwTotal];
    res->last = hw[kLwLast];
    res->bad = hw[kLwBadIndex];
    res->sel[0] = hw[kLwSel];
    res->sel[1] = hw[kLwSel + 1];
    FCX_TRY(T.add(3, 4));
    T.publish(c, kLStageNames, kLStages);
    return FCX_OK;
}

namespace {

bool kind_ok(char kind) { return kind == '7' || kind == '8'; }

// the four values of FCX_LINES_STATS from a whole count
void line_stats(uint64_t nl, uint64_t last, uint64_t total, uint64_t *stats) {
    stats[0] = nl;
    stats[1] = nl + (total > 0 && last != total);
    stats[2] = total;
    stats[3] = total - std::min(last, total);
}

// the two ranks a locate asks for: lines [first, end) lie between the first-th and the end-th delimiter
struct Bounds {
    uint64_t first, end;
};
Bounds bounds_of(uint64_t first, uint64_t count) { return {first, count < ~0ull - first ? first + count : ~0ull}; }

// 1 + the position of the r-th delimiter as a select left it (r == 0: the start of the run), T when the run
// does not hold it
uint64_t start_of(uint64_t r, uint64_t sel, uint64_t total) { return r == 0 ? 0 : sel == kLNone ? total : sel; }

int format_index(uint64_t rec, const char *why) {
    return fail(FCX_ERR_FORMAT, "fcx_lines_locate_shard: the index disagrees with the run: record " + std::to_string(rec) + " " + why);
}

// The locate over a caller's index: its arrays on the host, the records of the two delimiters by bisection,
// each decoded alone through the range decode (which holds every touched record to the index's size and stays
// inside the run) and scanned.
int locate_indexed(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                   const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_line_off, Bounds b, uint64_t *off,
                   uint64_t *len, hipStream_t st) {
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    LinesScratch &S = c->ln;
    VerifyScratch &V = c->vf;
    c->times.reset();   // (no stage table: this path has no index or group stage of its own)
    std::vector<uint64_t> roff(nblocks + 1), doff(nblocks + 1), loff(nblocks + 1);
    FCX_HIP(hipMemcpyAsync(roff.data(), d_rec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemcpyAsync(doff.data(), d_dec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipMemcpyAsync(loff.data(), d_line_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    if (roff[0] || doff[0] || loff[0]) return format_index(0, "does not start at 0");
    for (uint32_t k = 0; k < nblocks; k++) {
        if (roff[k + 1] < roff[k] || doff[k + 1] < doff[k] || loff[k + 1] < loff[k]) return format_index(k, "is behind the next one");
        if (doff[k + 1] - doff[k] > FCX_MAX_BLOCK_BYTES + 8ull) return format_index(k, "is larger than a block");
        if (loff[k + 1] - loff[k] > doff[k + 1] - doff[k]) return format_index(k, "has more delimiters than bytes");
    }
    const uint64_t total = doff[nblocks], nl = loff[nblocks];
    const uint64_t r[2] = {b.first, b.end};
    uint64_t sel[2] = {kLNone, kLNone};
    uint32_t rec[2] = {~0u, ~0u};
    for (int q = 0; q < 2; q++) {
        if (r[q] == 0 || r[q] > nl || r[q] <= loff[0]) continue;
        // the record k with line_off[k] < r <= line_off[k + 1]
        rec[q] = (uint32_t)(std::lower_bound(loff.begin() + 1, loff.end(), r[q]) - loff.begin()) - 1;
    }
    for (int q = 0; q < 2; q++) {
        if (rec[q] == ~0u || (q == 1 && rec[1] == rec[0])) continue;
        const uint32_t k = rec[q];
        const uint64_t size = doff[k + 1] - doff[k];
        FCX_TRY(V.buf.reserve(size + 64, "verify buffer"));
        FCX_TRY(chunk_room(S, size));
        uint64_t got = 0;
        FCX_TRY(range_shard(c, kind, d_rec, rec_len, nblocks, d_rec_off, d_dec_off, doff[k], size, V.buf, size, &got, st, 0, nullptr));
        if (got != size) return format_index(k, "does not decode to the index's bytes");
        LinesReq at;
        at.nl_before = loff[k];
        uint64_t w0[kLwWords];
        preset(w0, at);
        FCX_HIP(hipMemcpyAsync(S.words, w0, 8 * kLwWords, hipMemcpyHostToDevice, st));
        launch_count(S, V.buf, size, delim, doff[k], st);
        const uint64_t want[2] = {r[q], q == 0 && rec[1] == k ? r[1] : kLNone};
        launch_select(S, V.buf, size, delim, doff[k], want, st);
        FCX_HIP(hipGetLastError());
        FCX_HIP(hipMemcpyAsync(S.host_words, S.words, 8 * kLwWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));   // (`w0` may go)
        const uint64_t *hw = S.host_words;
        S.stats[0] += hw[kLwBytes];
        S.stats[1]++;
        S.stats[2]++;
        if (hw[kLwTotal] != loff[k + 1] || hw[kLwSel] == kLNone || (want[1] != kLNone && hw[kLwSel + 1] == kLNone))
            return format_index(k, "does not hold the delimiters the line index promises");
        sel[q] = hw[kLwSel];
        if (want[1] != kLNone) sel[1] = hw[kLwSel + 1];
    }
    c->times.reset();   // (not the inner range decode's table either)
    *off = start_of(b.first, sel[0], total);
    *len = start_of(b.end, sel[1], total) - *off;
    return FCX_OK;
}

// fcx_lines_locate_shard behind its argument checks; with no index given the run's own stays in the range
// API's scratch (rg.rec_off, rg.dec_off) for a range decode that follows
int locate_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                 const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_line_off, uint64_t first, uint64_t count,
                 uint64_t *off, uint64_t *len, hipStream_t st) {
    *off = *len = 0;
    const Bounds b = bounds_of(first, count);
    if (nblocks == 0) {
        for (uint64_t &v : c->ln.stats) v = 0;
        return FCX_OK;
    }
    if (d_rec_off) return locate_indexed(c, kind, d_rec, rec_len, nblocks, delim, d_rec_off, d_dec_off, d_line_off, b, off, len, st);
    LinesReq q;
    q.delim = delim;
    q.stop_early = true;
    // a run of T bytes holds T delimiters at most: a rank beyond needs no search (the run's size is the index's)
    q.staged = [&](uint64_t decoded, LinesReq *r) {
        r->sel[0] = b.first && b.first <= decoded ? b.first : kLNone;
        r->sel[1] = b.end && b.end <= decoded ? b.end : kLNone;
        return FCX_OK;
    };
    LinesRes res;
    FCX_TRY(lines_run(c, kind, d_rec, rec_len, nblocks, q, &res, st, 0));
    *off = start_of(b.first, res.sel[0], res.decoded);
    *len = start_of(b.end, res.sel[1], res.decoded) - *off;
    return FCX_OK;
}

}  // namespace
}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_lines_index_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                          uint64_t *d_line_off, uint64_t *stats, void *stream) {
    if (!c || !stats || (nblocks && !d_rec)) return fail(FCX_ERR_ARG, "fcx_lines_index_shard: NULL argument");
    if (!kind_ok(kind)) return fail(FCX_ERR_ARG, "fcx_lines_index_shard: kind must be '7' or '8'");
    for (int i = 0; i < FCX_LINES_STATS; i++) stats[i] = 0;
    if (nblocks == 0) {
        for (uint64_t &v : c->ln.stats) v = 0;
        return FCX_OK;
    }
    LinesReq q;
    q.delim = delim;
    q.d_line_off = d_line_off;
    LinesRes res;
    FCX_TRY(lines_run(c, kind, d_rec, rec_len, nblocks, q, &res, (hipStream_t)stream, 0));
    line_stats(res.nl, res.last, res.decoded, stats);
    return FCX_OK;
}

int fcx_lines_locate_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                           const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_line_off, uint64_t first,
                           uint64_t count, uint64_t *off, uint64_t *len, void *stream) {
    if (!c || !off || !len || (nblocks && !d_rec)) return fail(FCX_ERR_ARG, "fcx_lines_locate_shard: NULL argument");
    if (!kind_ok(kind)) return fail(FCX_ERR_ARG, "fcx_lines_locate_shard: kind must be '7' or '8'");
    if (!d_rec_off != !d_dec_off || !d_rec_off != !d_line_off)
        return fail(FCX_ERR_ARG, "fcx_lines_locate_shard: a part of an index (some pointers NULL)");
    return locate_shard(c, kind, d_rec, rec_len, nblocks, delim, d_rec_off, d_dec_off, d_line_off, first, count, off, len,
                        (hipStream_t)stream);
}

int fcx_decompress_lines_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                               const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_line_off, uint64_t first,
                               uint64_t count, uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream) {
    if (!c || !out_len || (nblocks && !d_rec) || (cap && !d_out)) return fail(FCX_ERR_ARG, "fcx_decompress_lines_shard: NULL argument");
    if (!kind_ok(kind)) return fail(FCX_ERR_ARG, "fcx_decompress_lines_shard: kind must be '7' or '8'");
    if (!d_rec_off != !d_dec_off || !d_rec_off != !d_line_off)
        return fail(FCX_ERR_ARG, "fcx_decompress_lines_shard: a part of an index (some pointers NULL)");
    hipStream_t st = (hipStream_t)stream;
    uint64_t off = 0, len = 0;
    *out_len = 0;
    FCX_TRY(locate_shard(c, kind, d_rec, rec_len, nblocks, delim, d_rec_off, d_dec_off, d_line_off, first, count, &off, &len, st));
    *out_len = len;
    if (len > cap) return fail(FCX_ERR_CAPACITY, "fcx_decompress_lines_shard: output capacity too small");
    if (len == 0) return FCX_OK;
    // the index the locate built is still in the range API's scratch
    const uint64_t *ro = d_rec_off ? d_rec_off : (const uint64_t *)c->rg.rec_off, *dof = d_rec_off ? d_dec_off : (const uint64_t *)c->rg.dec_off;
    uint64_t got = 0;
    FCX_TRY(range_shard(c, kind, d_rec, rec_len, nblocks, ro, dof, off, len, d_out, len, &got, st, 0, nullptr));
    if (got != len) return fail(FCX_ERR_FORMAT, "fcx_decompress_lines_shard: the index disagrees with the run");
    return FCX_OK;
}

int fcx_lines_of_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                       const uint64_t *d_offsets, uint64_t noff, uint64_t *d_lines, void *stream) {
    if (!c || (nblocks && !d_rec) || (noff && (!d_offsets || !d_lines))) return fail(FCX_ERR_ARG, "fcx_lines_of_shard: NULL argument");
    if (!kind_ok(kind)) return fail(FCX_ERR_ARG, "fcx_lines_of_shard: kind must be '7' or '8'");
    if (noff == 0) {
        for (uint64_t &v : c->ln.stats) v = 0;
        return FCX_OK;
    }
    LinesReq q;
    q.delim = delim;
    q.d_offsets = d_offsets;
    q.noff = noff;
    q.d_lines = d_lines;
    q.check_offsets = true;
    LinesRes res;
    FCX_TRY(lines_run(c, kind, d_rec, rec_len, nblocks, q, &res, (hipStream_t)stream, 0));
    if (res.bad != kLNone)
        return fail(FCX_ERR_ARG, "fcx_lines_of_shard: offset " + std::to_string(res.bad) + " descends or lies behind the run's end");
    return FCX_OK;
}

int fcx_dctx_lines_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_lines_stats: bad argument");
    for (int i = 0; i < n && i < FCX_LINES_CALL_STATS; i++) out[i] = c->ln.stats[i];
    return FCX_OK;
}

}  // extern "C"
