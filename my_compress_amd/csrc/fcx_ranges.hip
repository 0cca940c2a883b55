// fcx_ranges.hip — batched random access into a device-resident run (gfx950): many ascending byte ranges of
// what the records decode to, concatenated, in one call.  fcx_decompress_ranges_shard of include/fcx.h, and
// the host forms fcx_decompress_ranges_host and fcx_grep_host (fcx_grep_shard's arrays chained into it).
// DESIGN.md §9i.
//
// The ranges stay on the device.  What the host learns of them is their sum, the first one that breaks a
// rule, and one flag per record.
//   k_qlen       a thread per range: the rules (start <= end <= T, end of the one before <= start) and the
//                length; per chunk of 1024 ranges their sum.
//   k_qchunks    one workgroup: the exclusive scan of the chunk sums (any number of chunks), the total.
//   k_qoff       per chunk again: out_off[i] = the bytes of the ranges before i (nranges + 1 values).
//   k_qtouch     a thread per record: does a range hold a byte of it?  Two bisections over the ranges (the ends
//                ascend as the starts do) and a difference of out_off, which skips the empty ranges between.
//                Per record, not per range, so one range over a million records costs no thread a million
//                stores.
//   the groups   fcx_verify_shard's; of each only the touched records are decoded, stretch by stretch, to their
//                places in the bounded buffer; a group without one is skipped.
//   k_qslice     one thread per decoded group: the ranges [ia, ib) that meet it and its span of the output.
//   k_qgather    output-driven: a lane per 16 bytes of the output, aligned to the destination.  It bisects
//                out_off within [ia, ib) for the range of its first byte.  Where the 16 bytes lie in one range
//                they are read through ld16_bounded (the source sits anywhere) and stored as one
//                global_store_dwordx4; where they cross ranges (short lines) they are collected byte by byte
//                and still stored once; only the two ragged ends of the group's span are stored by bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"

namespace fcx {

constexpr uint32_t kQThreads = 256;
constexpr uint32_t kQChunk = 1024;      // ranges per workgroup of k_qlen / k_qoff
constexpr uint32_t kQMaxGrid = 2048;    // workgroups of k_qgather at most
constexpr uint64_t kQNone = ~0ull;

// block-wide exclusive scan of u64 (blockDim.x threads, <= 16 waves); the total in *tot
__device__ inline uint64_t block_xscan64(uint64_t v, uint64_t *sh, uint64_t *tot) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += u;
    }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    uint64_t pre = inc - v, all = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint64_t x = sh[w];
        if (w < wv) pre += x;
        all += x;
    }
    __syncthreads();
    *tot = all;
    return pre;
}

// the length of range i, 0 for one that breaks a rule: its index then goes to kQwBadIndex by an atomic minimum
__device__ inline uint64_t range_len(const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t i, uint64_t total,
                                     uint64_t *words) {
    const uint64_t s = start[i], e = end[i];
    if (s > e || e > total || (i > 0 && end[i - 1] > s)) {
        if (words) atomicMin((unsigned long long *)words + kQwBadIndex, (unsigned long long)i);
        return 0;
    }
    return e - s;
}

__global__ __launch_bounds__(kQChunk) void k_qlen(const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t n,
                                                  uint64_t total, uint64_t *__restrict__ chunk_sum, uint64_t *__restrict__ words) {
    __shared__ uint64_t sh[kQChunk / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kQChunk + threadIdx.x;
    uint64_t tot;
    block_xscan64(i < n ? range_len(start, end, i, total, words) : 0, sh, &tot);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = tot;
}

// chunk_sum[k] becomes the bytes of the chunks before k; words[kQwSum]: the bytes of all
__global__ __launch_bounds__(1024) void k_qchunks(uint64_t *__restrict__ chunk_sum, uint64_t nchunks, uint64_t *__restrict__ words) {
    __shared__ uint64_t sh[16];
    uint64_t carry = 0;
    for (uint64_t k0 = 0; k0 < nchunks; k0 += 1024) {
        const uint64_t k = k0 + threadIdx.x;
        uint64_t tot;
        const uint64_t pre = block_xscan64(k < nchunks ? chunk_sum[k] : 0, sh, &tot);
        if (k < nchunks) chunk_sum[k] = carry + pre;
        carry += tot;
    }
    if (threadIdx.x == 0) words[kQwSum] = carry;
}

__global__ __launch_bounds__(kQChunk) void k_qoff(const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t n,
                                                  uint64_t total, const uint64_t *__restrict__ chunk_sum, uint64_t *__restrict__ out_off) {
    __shared__ uint64_t sh[kQChunk / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kQChunk + threadIdx.x;
    const uint64_t len = i < n ? range_len(start, end, i, total, nullptr) : 0;
    uint64_t tot;
    const uint64_t pre = chunk_sum[blockIdx.x] + block_xscan64(len, sh, &tot);
    if (i < n) out_off[i] = pre;
    if (i + 1 == n) out_off[n] = pre + len;
}

// the first i in [0, n) with a[i] > x when a ascends (n: none)
__device__ inline uint64_t first_above(const uint64_t *__restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the ranges that can hold a byte of [lo, hi), lo < hi: [*ia, *ib) = those with end > lo and start < hi
__device__ inline void ranges_meeting(const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t n, uint64_t lo,
                                      uint64_t hi, uint64_t *ia, uint64_t *ib) {
    *ia = first_above(end, n, lo);
    *ib = first_above(start, n, hi - 1);
}

// touched[r] = 1 iff a range holds a byte of record r; words[kQwTouched]: how many
__global__ __launch_bounds__(kQThreads) void k_qtouch(uint32_t nblocks, const uint64_t *__restrict__ dec_off,
                                                      const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t n,
                                                      const uint64_t *__restrict__ out_off, uint8_t *__restrict__ touched,
                                                      uint64_t *__restrict__ words) {
    const uint32_t r = blockIdx.x * kQThreads + threadIdx.x;
    uint32_t hit = 0;
    if (r < nblocks) {
        const uint64_t lo = dec_off[r], hi = dec_off[r + 1];
        if (lo < hi) {
            uint64_t ia, ib;
            ranges_meeting(start, end, n, lo, hi, &ia, &ib);
            hit = ia < ib && out_off[ib] > out_off[ia];   // (not only empty ranges)
        }
        touched[r] = (uint8_t)hit;
    }
    const uint64_t m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long *)words + kQwTouched, (unsigned long long)__popcll(m));
}

// one thread: words[kQwSlice ..] = the ranges [ia, ib) that meet the decoded bytes [g_lo, g_hi) and the span
// [o_lo, o_hi) of the output their pieces inside fill (empty: o_lo == o_hi)
__global__ void k_qslice(const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t n,
                         const uint64_t *__restrict__ out_off, uint64_t g_lo, uint64_t g_hi, uint64_t *__restrict__ words) {
    uint64_t ia = 0, ib = 0, o_lo = 0, o_hi = 0;
    if (g_lo < g_hi) {
        ranges_meeting(start, end, n, g_lo, g_hi, &ia, &ib);
        if (ia < ib) {
            const uint64_t s0 = start[ia], s1 = start[ib - 1], e1 = min(end[ib - 1], g_hi);
            o_lo = out_off[ia] + (g_lo > s0 ? g_lo - s0 : 0);
            o_hi = out_off[ib - 1] + (e1 > s1 ? e1 - s1 : 0);
        }
    }
    words[kQwSlice] = ia;
    words[kQwSlice + 1] = ib;
    words[kQwSlice + 2] = o_lo;
    words[kQwSlice + 3] = o_hi < o_lo ? o_lo : o_hi;
}

// The group decoded at [buf, buf + gbytes) holds the run's bytes from g_lo on: the output bytes [o_lo, o_hi) of
// k_qslice are copied from it.  Nothing outside [buf, buf + gbytes) is read, nothing outside d_out[o_lo, o_hi)
// written.
__global__ __launch_bounds__(kQThreads) void k_qgather(const uint8_t *__restrict__ buf, uint64_t gbytes, uint64_t g_lo,
                                                       const uint64_t *__restrict__ start, const uint64_t *__restrict__ out_off,
                                                       const uint64_t *__restrict__ words, uint8_t *__restrict__ d_out) {
    const uint64_t ia = words[kQwSlice], ib = words[kQwSlice + 1], o_lo = words[kQwSlice + 2], o_hi = words[kQwSlice + 3];
    if (o_lo >= o_hi || ia >= ib) return;
    // q = output offset + a is 16-byte aligned where the destination is
    const uint64_t a = (uintptr_t)d_out & 15, q_lo = o_lo + a, q_hi = o_hi + a;
    const uint64_t c_hi = (q_hi + 15) >> 4;
    for (uint64_t c = (q_lo >> 4) + (uint64_t)blockIdx.x * kQThreads + threadIdx.x; c < c_hi; c += (uint64_t)gridDim.x * kQThreads) {
        const uint64_t qa = max(16 * c, q_lo), qb = min(16 * c + 16, q_hi), o = qa - a;
        uint64_t lo = ia, hi = ib;   // the last i in [ia, ib) with out_off[i] <= o (out_off[ia] <= o_lo)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (out_off[mid] <= o) lo = mid;
            else hi = mid;
        }
        uint64_t i = lo, next = out_off[i + 1];
        const bool whole = qb - qa == 16;
        uint4 w;
        if (whole && next - o >= 16) {
            const uint64_t x = start[i] + (o - out_off[i]) - g_lo;
            w = ld16_bounded(buf, x, (uint32_t)((uintptr_t)(buf + x) & 15), gbytes);
        } else {
            uint32_t acc[4] = {0, 0, 0, 0};
            uint64_t from = start[i] - out_off[i] - g_lo;   // source position in buf = output offset + from (mod 2^64)
            for (uint64_t q = qa; q < qb; q++) {
                const uint64_t oo = q - a;
                while (oo >= next) {
                    i++;
                    next = out_off[i + 1];
                    from = start[i] - out_off[i] - g_lo;
                }
                const uint32_t byte = buf[oo + from];
                if (whole) acc[(q & 15) >> 2] |= byte << (8 * (q & 3));
                else d_out[oo] = (uint8_t)byte;
            }
            if (!whole) continue;
            w = make_uint4(acc[0], acc[1], acc[2], acc[3]);
        }
        *(uint4 *)(d_out + o) = w;
    }
}

namespace {
const char *kQStageNames[] = {"index", "map", "decode", "gather"};
constexpr int kQStages = 4;
const char *const kQWho = "fcx_decompress_ranges_shard";

int ready(fcx_dctx *c) {
    RangesScratch &Q = c->rq;
    if (!Q.host_words) {
        FCX_TRY(Q.words.reserve(8 * kQwWords, "ranges words"));
        FCX_HIP(Q.host_words.alloc(8 * kQwWords));
    }
    return FCX_OK;
}

int format_index(uint64_t rec, const char *why) {
    return fail(FCX_ERR_FORMAT, std::string(kQWho) + ": the index disagrees with the run: record " + std::to_string(rec) + " " + why);
}
}  // namespace

int ranges_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint64_t *d_rec_off,
               const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end, uint64_t nranges, uint8_t *d_out,
               uint64_t cap, uint64_t *out_len, hipStream_t st) {
    RangesScratch &Q = c->rq;
    *out_len = 0;
    for (uint64_t &v : Q.stats) v = 0;
    if (nranges == 0) return FCX_OK;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    VerifyScratch &V = c->vf;
    RunTimes T(c, kQStages, st);
    RunIndex ix;
    const bool given = d_rec_off != nullptr;
    if (nblocks == 0) {
        T.mark(0);
        T.mark(1);
        ix.roff.assign(1, 0);
        ix.doff.assign(1, 0);
    } else if (given) {
        T.mark(0);
        ix.roff.resize(nblocks + 1);
        ix.doff.resize(nblocks + 1);
        FCX_HIP(hipMemcpyAsync(ix.roff.data(), d_rec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipMemcpyAsync(ix.doff.data(), d_dec_off, 8ull * nblocks + 8, hipMemcpyDeviceToHost, st));
        T.mark(1);
    } else {
        FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
        d_dec_off = c->rg.dec_off;
    }
    FCX_HIP(hipMemsetAsync(Q.words, 0, 8 * kQwWords, st));
    FCX_HIP(hipMemsetAsync((uint64_t *)Q.words + kQwBadIndex, 0xFF, 8, st));
    FCX_HIP(hipStreamSynchronize(st));   // (the index is on the host)
    FCX_TRY(T.add(0, 1));
    const std::vector<uint64_t> &roff = ix.roff, &doff = ix.doff;
    if (given && nblocks) {   // where a caller's index points must be inside the run
        if (roff[0] || doff[0]) return format_index(0, "does not start at 0");
        for (uint32_t k = 0; k < nblocks; k++) {
            if (roff[k + 1] < roff[k] + 4 || doff[k + 1] < doff[k]) return format_index(k, "is behind the next one");
            if (doff[k + 1] - doff[k] > FCX_MAX_BLOCK_BYTES + 8ull) return format_index(k, "is larger than a block");
        }
        if (roff[nblocks] > rec_len) return format_index(nblocks - 1, "ends behind the run");
    }
    const uint64_t total = doff[nblocks];
    // the map: lengths, output offsets, touched records
    const uint64_t nchunks = (nranges + kQChunk - 1) / kQChunk;
    if (nchunks > 0x7FFFFFFFull) return fail(FCX_ERR_ARG, std::string(kQWho) + ": more than 2^41 ranges");
    FCX_TRY(Q.out_off.reserve(8 * nranges + 8, "range offsets"));
    FCX_TRY(Q.chunk_sum.reserve(8 * nchunks, "range chunk sums"));
    FCX_TRY(Q.touched.reserve(nblocks, "touched records"));
    if (!Q.host_touched || Q.host_touched.bytes < nblocks) FCX_HIP(Q.host_touched.alloc(nblocks));
    T.mark(1);
    hipLaunchKernelGGL(k_qlen, dim3((uint32_t)nchunks), dim3(kQChunk), 0, st, d_start, d_end, nranges, total, (uint64_t *)Q.chunk_sum,
                       (uint64_t *)Q.words);
    hipLaunchKernelGGL(k_qchunks, dim3(1), dim3(1024), 0, st, (uint64_t *)Q.chunk_sum, nchunks, (uint64_t *)Q.words);
    hipLaunchKernelGGL(k_qoff, dim3((uint32_t)nchunks), dim3(kQChunk), 0, st, d_start, d_end, nranges, total,
                       (const uint64_t *)Q.chunk_sum, (uint64_t *)Q.out_off);
    if (nblocks) {
        hipLaunchKernelGGL(k_qtouch, dim3((nblocks + kQThreads - 1) / kQThreads), dim3(kQThreads), 0, st, nblocks, d_dec_off, d_start,
                           d_end, nranges, (const uint64_t *)Q.out_off, (uint8_t *)Q.touched, (uint64_t *)Q.words);
        FCX_HIP(hipMemcpyAsync(Q.host_touched, Q.touched, nblocks, hipMemcpyDeviceToHost, st));
    }
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(Q.host_words, Q.words, 8 * kQwWords, hipMemcpyDeviceToHost, st));
    T.mark(2);
    FCX_HIP(hipStreamSynchronize(st));
    FCX_TRY(T.add(1, 2));
    const uint64_t bad = Q.host_words[kQwBadIndex], sum = Q.host_words[kQwSum];
    if (bad != kQNone)
        return fail(FCX_ERR_ARG, std::string(kQWho) + ": range " + std::to_string(bad) +
                                     " breaks start <= end <= decoded bytes or starts in front of the end of the range before it");
    *out_len = sum;
    Q.stats[0] = nranges;
    Q.stats[2] = Q.host_words[kQwTouched];
    if (sum > cap) return fail(FCX_ERR_CAPACITY, std::string(kQWho) + ": output capacity too small");
    const uint8_t *touched = Q.host_touched;
    std::vector<RunGroup> groups;
    const auto any = [&](uint32_t g0, uint32_t g1) { return std::find(touched + g0, touched + g1, 1) != touched + g1; };
    if (nblocks && sum) FCX_TRY(run_groups(c, ix, nblocks, &groups, any));
    for (const RunGroup &g : groups) {
        if (!any(g.g0, g.g1)) continue;
        uint32_t a = g.g0, b = g.g1;   // from the group's first to its last touched record
        while (!touched[a]) a++;
        while (!touched[b - 1]) b--;
        const uint64_t want = doff[b] - doff[a];
        T.mark(2);
        // every stretch of touched records to its place in the buffer; what lies between is neither decoded nor read
        for (uint32_t r0 = a; r0 < b;) {
            if (!touched[r0]) {
                r0++;
                continue;
            }
            uint32_t r1 = r0 + 1;
            while (r1 < b && touched[r1]) r1++;
            const uint64_t part = doff[r1] - doff[r0], at = roff[r0];
            uint8_t *dst = V.buf + (doff[r0] - doff[a]);
            uint64_t got = 0;
            if (kind == '7') FCX_TRY(fcx_decompress_shard(c, d_rec + at, rec_len - at, r1 - r0, dst, part, &got, st));
            else FCX_TRY(lz78_decompress_shard_at(c, d_rec + at, rec_len - at, r1 - r0, dst, part, &got, st, r0));
            if (got != part)
                return given ? format_index(r0, "and the touched ones behind it do not decode to the index's bytes")
                             : fail(FCX_ERR_INTERNAL, std::string(kQWho) + ": the decode of a group disagrees with the index");
            Q.stats[3] += r1 - r0;
            r0 = r1;
        }
        T.mark(3);
        hipLaunchKernelGGL(k_qslice, dim3(1), dim3(1), 0, st, d_start, d_end, nranges, (const uint64_t *)Q.out_off, doff[a], doff[b],
                           (uint64_t *)Q.words);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((want / 16 + kQThreads) / kQThreads, kQMaxGrid);
        hipLaunchKernelGGL(k_qgather, dim3(grid), dim3(kQThreads), 0, st, (const uint8_t *)V.buf, want, doff[a], d_start,
                           (const uint64_t *)Q.out_off, (const uint64_t *)Q.words, d_out);
        T.mark(4);
        FCX_HIP(hipGetLastError());
        FCX_TRY(T.add(2, 4));
        Q.stats[4]++;
    }
    FCX_HIP(hipStreamSynchronize(st));
    Q.stats[1] = sum;
    T.publish(c, kQStageNames, kQStages);
    return FCX_OK;
}

namespace {

// A whole file in host memory: its kind, and its records (no header) counted.  FCX7 reads records to the end
// of the file, FCX8 the header's count, as the stream forms do.
int walk_file(const uint8_t *in, uint64_t in_len, char *kind, uint32_t *nblocks, uint64_t *rec_len) {
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    uint32_t total = 0;
    uint16_t counted = 0;
    char k = 0;
    FCX_TRY(fcx_parse_header(in, &total, &counted, &k));
    const bool lz78 = k != '7';
    const uint64_t len_max = lz78 ? 10ull * FCX_MAX_BLOCK_BYTES + 4096 : 2ull * FCX_MAX_BLOCK_BYTES + 4096;
    uint64_t at = FCX_HEADER_BYTES, n = 0;
    while (lz78 ? n < counted : at < in_len) {
        uint32_t len = 0;
        if (in_len - at < 4) return fail(FCX_ERR_FORMAT, "truncated block record");
        memcpy(&len, in + at, 4);
        if (len > len_max) return fail(FCX_ERR_FORMAT, "block record too long");
        if (in_len - at - 4 < len) return fail(FCX_ERR_FORMAT, "truncated block record");
        at += 4 + (uint64_t)len;
        if (++n > 0x7FFFFFFFull) return fail(FCX_ERR_FORMAT, "too many block records");
    }
    *kind = lz78 ? '8' : '7';
    *nblocks = (uint32_t)n;
    *rec_len = at - FCX_HEADER_BYTES;
    return FCX_OK;
}

// the file's records to the device (rq.file), on the null stream
int stage_file(fcx_dctx *c, const uint8_t *in, uint64_t rec_len) {
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(c->rq.file.reserve(rec_len, "file records"));
    if (rec_len) FCX_HIP(hipMemcpy(c->rq.file, in + FCX_HEADER_BYTES, rec_len, hipMemcpyHostToDevice));
    return FCX_OK;
}

// d_out[0, n) of rq.out to the caller
int fetch_out(fcx_dctx *c, uint8_t *out, uint64_t n) {
    if (n) FCX_HIP(hipMemcpy(out, c->rq.out, n, hipMemcpyDeviceToHost));
    return FCX_OK;
}

constexpr uint64_t kQGuessLines = 1u << 16;   // lines fcx_grep_host gives room for before it knows their number

}  // namespace
}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_decompress_ranges_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                                const uint64_t *d_rec_off, const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end,
                                uint64_t nranges, uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream) {
    if (!c || !out_len || (nblocks && !d_rec) || (nranges && (!d_start || !d_end)) || (cap && !d_out))
        return fail(FCX_ERR_ARG, "fcx_decompress_ranges_shard: NULL argument");
    if (kind != '7' && kind != '8') return fail(FCX_ERR_ARG, "fcx_decompress_ranges_shard: kind must be '7' or '8'");
    if (!d_rec_off != !d_dec_off) return fail(FCX_ERR_ARG, "fcx_decompress_ranges_shard: half an index (one pointer NULL)");
    return ranges_run(c, kind, d_rec, rec_len, nblocks, d_rec_off, d_dec_off, d_start, d_end, nranges, d_out, cap, out_len,
                      (hipStream_t)stream);
}

int fcx_dctx_ranges_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_ranges_stats: bad argument");
    for (int i = 0; i < n && i < FCX_RANGES_STATS; i++) out[i] = c->rq.stats[i];
    return FCX_OK;
}

int fcx_decompress_ranges_host(fcx_dctx *c, const uint8_t *in, uint64_t in_len, const uint64_t *starts, const uint64_t *ends,
                               uint64_t nranges, uint8_t *out, uint64_t cap, uint64_t *out_len) {
    if (!c || !in || !out_len || (nranges && (!starts || !ends)) || (cap && !out))
        return fail(FCX_ERR_ARG, "fcx_decompress_ranges_host: NULL argument");
    char kind = 0;
    uint32_t nblocks = 0;
    uint64_t rec_len = 0;
    FCX_TRY(walk_file(in, in_len, &kind, &nblocks, &rec_len));
    *out_len = 0;
    if (nranges == 0) return FCX_OK;
    RangesScratch &Q = c->rq;
    FCX_TRY(stage_file(c, in, rec_len));
    FCX_TRY(Q.starts.reserve(8 * nranges, "ranges"));
    FCX_TRY(Q.ends.reserve(8 * nranges, "ranges"));
    FCX_TRY(Q.out.reserve(cap, "ranges output"));
    FCX_HIP(hipMemcpy(Q.starts, starts, 8 * nranges, hipMemcpyHostToDevice));
    FCX_HIP(hipMemcpy(Q.ends, ends, 8 * nranges, hipMemcpyHostToDevice));
    FCX_TRY(ranges_run(c, kind, Q.file, rec_len, nblocks, nullptr, nullptr, Q.starts, Q.ends, nranges, cap ? (uint8_t *)Q.out : nullptr, cap,
                       out_len, nullptr));
    return fetch_out(c, out, *out_len);
}

// fcx_decompress_ranges_host with the cut behind the gather: only the cut bytes come back
int fcx_cut_ranges_host(fcx_dctx *c, const uint8_t *in, uint64_t in_len, const uint64_t *starts, const uint64_t *ends, uint64_t nranges,
                        const fcx_cut *cut, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats) {
    if (!c || !in || !cut || !out_len || (nranges && (!starts || !ends)) || (cap && !out))
        return fail(FCX_ERR_ARG, "fcx_cut_ranges_host: NULL argument");
    char kind = 0;
    uint32_t nblocks = 0;
    uint64_t rec_len = 0;
    FCX_TRY(walk_file(in, in_len, &kind, &nblocks, &rec_len));
    *out_len = 0;
    for (int i = 0; i < FCX_CUT_STATS && stats; i++) stats[i] = 0;
    if (nranges == 0) return cut_ranges_run(c, kind, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, cut, nullptr, 0, out_len, stats, nullptr);
    RangesScratch &Q = c->rq;
    FCX_TRY(stage_file(c, in, rec_len));
    FCX_TRY(Q.starts.reserve(8 * nranges, "ranges"));
    FCX_TRY(Q.ends.reserve(8 * nranges, "ranges"));
    FCX_TRY(c->ct.out.reserve(cap, "cut output"));
    FCX_HIP(hipMemcpy(Q.starts, starts, 8 * nranges, hipMemcpyHostToDevice));
    FCX_HIP(hipMemcpy(Q.ends, ends, 8 * nranges, hipMemcpyHostToDevice));
    FCX_TRY(cut_ranges_run(c, kind, Q.file, rec_len, nblocks, nullptr, nullptr, Q.starts, Q.ends, nranges, cut,
                           cap ? (uint8_t *)c->ct.out : nullptr, cap, out_len, stats, nullptr));
    if (*out_len > cap) return fail(FCX_ERR_CAPACITY, "fcx_cut_ranges_host: output capacity too small");
    if (*out_len) FCX_HIP(hipMemcpy(out, c->ct.out, *out_len, hipMemcpyDeviceToHost));
    return FCX_OK;
}

int fcx_grep_host(fcx_dctx *c, const uint8_t *in, uint64_t in_len, uint8_t delim, const uint8_t *pattern, uint32_t plen, uint8_t *out,
                  uint64_t cap, uint64_t *out_len, uint64_t *stats) {
    if (!c || !in || !pattern || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_grep_host: NULL argument");
    if (plen < 1 || plen > FCX_FIND_MAX_PATTERN) return fail(FCX_ERR_ARG, "fcx_grep_host: pattern length outside [1, FCX_FIND_MAX_PATTERN]");
    if (memchr(pattern, delim, plen)) return fail(FCX_ERR_ARG, "fcx_grep_host: the pattern holds the delimiter");
    char kind = 0;
    uint32_t nblocks = 0;
    uint64_t rec_len = 0;
    FCX_TRY(walk_file(in, in_len, &kind, &nblocks, &rec_len));
    uint64_t gs[FCX_GREP_STATS] = {};
    *out_len = 0;
    for (int i = 0; i < FCX_GREP_STATS && stats; i++) stats[i] = 0;
    if (nblocks == 0) return FCX_OK;
    RangesScratch &Q = c->rq;
    FCX_TRY(stage_file(c, in, rec_len));
    // room for the lines: what the context holds already or a guess, and once more when the run has more
    uint64_t room = std::max<uint64_t>(std::min(Q.starts.bytes, Q.ends.bytes) / 8, kQGuessLines);
    for (int pass = 0; pass < 2; pass++) {
        FCX_TRY(Q.starts.reserve(8 * room, "ranges"));
        FCX_TRY(Q.ends.reserve(8 * room, "ranges"));
        GrepSink sink;
        sink.d_start = Q.starts;
        sink.d_end = Q.ends;
        sink.cap = room;
        FCX_TRY(grep_run(c, kind, Q.file, rec_len, nblocks, delim, pattern, plen, sink, nullptr, gs, nullptr, 0));
        if (gs[0] <= room) break;
        room = gs[0];
    }
    for (int i = 0; i < FCX_GREP_STATS && stats; i++) stats[i] = gs[i];
    *out_len = gs[1];
    if (gs[1] > cap) return fail(FCX_ERR_CAPACITY, "fcx_grep_host: output capacity too small");
    if (gs[1] == 0) return FCX_OK;
    FCX_TRY(Q.out.reserve(gs[1], "ranges output"));
    // the index the grep built is still in the range API's scratch
    uint64_t got = 0;
    FCX_TRY(ranges_run(c, kind, Q.file, rec_len, nblocks, c->rg.rec_off, c->rg.dec_off, Q.starts, Q.ends, gs[0], Q.out, gs[1], &got,
                       nullptr));
    if (got != gs[1]) return fail(FCX_ERR_INTERNAL, "fcx_grep_host: the lines' bytes disagree with the grep's sum");
    return fetch_out(c, out, got);
}

// fcx_grep_host for a pattern set: fcx_grep_set_shard's arrays chained into the multi-range decode
int fcx_grep_set_host(fcx_dctx *c, const uint8_t *in, uint64_t in_len, uint8_t delim, const fcx_pattern_set *set, uint8_t *out,
                      uint64_t cap, uint64_t *out_len, uint64_t *stats, uint64_t *counts) {
    if (!c || !in || !set || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_grep_set_host: NULL argument");
    FCX_TRY(set_args("fcx_grep_set_host", set, delim));
    char kind = 0;
    uint32_t nblocks = 0;
    uint64_t rec_len = 0;
    FCX_TRY(walk_file(in, in_len, &kind, &nblocks, &rec_len));
    uint64_t gs[FCX_GREP_STATS] = {};
    *out_len = 0;
    for (int i = 0; i < FCX_GREP_STATS && stats; i++) stats[i] = 0;
    GrepSink sink;
    if (nblocks == 0) return grep_set_run(c, kind, nullptr, 0, 0, delim, set, sink, nullptr, gs, counts, nullptr, 0);
    RangesScratch &Q = c->rq;
    FCX_TRY(stage_file(c, in, rec_len));
    // room for the lines: what the context holds already or a guess, and once more when the run has more
    uint64_t room = std::max<uint64_t>(std::min(Q.starts.bytes, Q.ends.bytes) / 8, kQGuessLines);
    for (int pass = 0; pass < 2; pass++) {
        FCX_TRY(Q.starts.reserve(8 * room, "ranges"));
        FCX_TRY(Q.ends.reserve(8 * room, "ranges"));
        sink.d_start = Q.starts;
        sink.d_end = Q.ends;
        sink.cap = room;
        FCX_TRY(grep_set_run(c, kind, Q.file, rec_len, nblocks, delim, set, sink, nullptr, gs, counts, nullptr, 0));
        if (gs[0] <= room) break;
        room = gs[0];
    }
    for (int i = 0; i < FCX_GREP_STATS && stats; i++) stats[i] = gs[i];
    *out_len = gs[1];
    if (gs[1] > cap) return fail(FCX_ERR_CAPACITY, "fcx_grep_set_host: output capacity too small");
    if (gs[1] == 0) return FCX_OK;
    FCX_TRY(Q.out.reserve(gs[1], "ranges output"));
    uint64_t got = 0;
    FCX_TRY(ranges_run(c, kind, Q.file, rec_len, nblocks, c->rg.rec_off, c->rg.dec_off, Q.starts, Q.ends, gs[0], Q.out, gs[1], &got,
                       nullptr));
    if (got != gs[1]) return fail(FCX_ERR_INTERNAL, "fcx_grep_set_host: the lines' bytes disagree with the grep's sum");
    return fetch_out(c, out, got);
}

// fcx_grep_set_host for blocks: fcx_grep_blocks_shard's starts and ends chained into the multi-range decode
int fcx_grep_blocks_host(fcx_dctx *c, const uint8_t *in, uint64_t in_len, uint8_t delim, const fcx_pattern_set *set,
                         const fcx_grep_opts *opts, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats, uint64_t *counts) {
    if (!c || !in || !set || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_grep_blocks_host: NULL argument");
    FCX_TRY(blocks_args("fcx_grep_blocks_host", set, delim, opts));
    char kind = 0;
    uint32_t nblocks = 0;
    uint64_t rec_len = 0;
    FCX_TRY(walk_file(in, in_len, &kind, &nblocks, &rec_len));
    uint64_t gs[FCX_GREP_BLOCK_STATS] = {};
    *out_len = 0;
    for (int i = 0; i < FCX_GREP_BLOCK_STATS && stats; i++) stats[i] = 0;
    BlockSink sink;
    if (nblocks == 0) return blocks_run(c, kind, nullptr, 0, 0, delim, set, *opts, sink, nullptr, gs, counts, nullptr, 0);
    RangesScratch &Q = c->rq;
    FCX_TRY(stage_file(c, in, rec_len));
    // room for the blocks: what the context holds already or a guess, and once more when the run has more
    uint64_t room = std::max<uint64_t>(std::min({Q.starts.bytes, Q.ends.bytes, c->cx.lines.bytes}) / 8, kQGuessLines);
    for (int pass = 0; pass < 2; pass++) {
        FCX_TRY(Q.starts.reserve(8 * room, "ranges"));
        FCX_TRY(Q.ends.reserve(8 * room, "ranges"));
        FCX_TRY(c->cx.lines.reserve(8 * room, "ranges"));
        sink.d_start = Q.starts;
        sink.d_end = Q.ends;
        sink.d_line = c->cx.lines;
        sink.cap = room;
        FCX_TRY(blocks_run(c, kind, Q.file, rec_len, nblocks, delim, set, *opts, sink, nullptr, gs, counts, nullptr, 0));
        if (gs[0] <= room) break;
        room = gs[0];
    }
    for (int i = 0; i < FCX_GREP_BLOCK_STATS && stats; i++) stats[i] = gs[i];
    *out_len = gs[2];
    if (gs[2] > cap) return fail(FCX_ERR_CAPACITY, "fcx_grep_blocks_host: output capacity too small");
    if (gs[2] == 0) return FCX_OK;
    FCX_TRY(Q.out.reserve(gs[2], "ranges output"));
    uint64_t got = 0;
    FCX_TRY(ranges_run(c, kind, Q.file, rec_len, nblocks, c->rg.rec_off, c->rg.dec_off, Q.starts, Q.ends, gs[0], Q.out, gs[2], &got,
                       nullptr));
    if (got != gs[2]) return fail(FCX_ERR_INTERNAL, "fcx_grep_blocks_host: the blocks' bytes disagree with the sum");
    return fetch_out(c, out, got);
}

// fcx_grep_blocks_host with the regex's run function
int fcx_grep_regex_blocks_host(fcx_dctx *c, const uint8_t *in, uint64_t in_len, const fcx_regex *re, const fcx_grep_opts *opts,
                               uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *stats) {
    if (!c || !in || !re || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_grep_regex_blocks_host: NULL argument");
    FCX_TRY(regex_args("fcx_grep_regex_blocks_host", re, opts));
    char kind = 0;
    uint32_t nblocks = 0;
    uint64_t rec_len = 0;
    FCX_TRY(walk_file(in, in_len, &kind, &nblocks, &rec_len));
    uint64_t gs[FCX_GREP_BLOCK_STATS] = {};
    *out_len = 0;
    for (int i = 0; i < FCX_GREP_BLOCK_STATS && stats; i++) stats[i] = 0;
    BlockSink sink;
    if (nblocks == 0) return regex_run(c, kind, nullptr, 0, 0, re, *opts, sink, nullptr, gs, nullptr, 0);
    RangesScratch &Q = c->rq;
    FCX_TRY(stage_file(c, in, rec_len));
    // room for the blocks: what the context holds already or a guess, and once more when the run has more
    uint64_t room = std::max<uint64_t>(std::min({Q.starts.bytes, Q.ends.bytes, c->cx.lines.bytes}) / 8, kQGuessLines);
    for (int pass = 0; pass < 2; pass++) {
        FCX_TRY(Q.starts.reserve(8 * room, "ranges"));
        FCX_TRY(Q.ends.reserve(8 * room, "ranges"));
        FCX_TRY(c->cx.lines.reserve(8 * room, "ranges"));
        sink.d_start = Q.starts;
        sink.d_end = Q.ends;
        sink.d_line = c->cx.lines;
        sink.cap = room;
        FCX_TRY(regex_run(c, kind, Q.file, rec_len, nblocks, re, *opts, sink, nullptr, gs, nullptr, 0));
        if (gs[0] <= room) break;
        room = gs[0];
    }
    for (int i = 0; i < FCX_GREP_BLOCK_STATS && stats; i++) stats[i] = gs[i];
    *out_len = gs[2];
    if (gs[2] > cap) return fail(FCX_ERR_CAPACITY, "fcx_grep_regex_blocks_host: output capacity too small");
    if (gs[2] == 0) return FCX_OK;
    FCX_TRY(Q.out.reserve(gs[2], "ranges output"));
    uint64_t got = 0;
    FCX_TRY(ranges_run(c, kind, Q.file, rec_len, nblocks, c->rg.rec_off, c->rg.dec_off, Q.starts, Q.ends, gs[0], Q.out, gs[2], &got,
                       nullptr));
    if (got != gs[2]) return fail(FCX_ERR_INTERNAL, "fcx_grep_regex_blocks_host: the blocks' bytes disagree with the sum");
    return fetch_out(c, out, got);
}

}  // extern "C"
