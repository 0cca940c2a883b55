// fcx_range.hip — random access into a device-resident run of FCX7 / FCX8 records (gfx950):
// the decoded-size index and the range decode of include/fcx.h.  DESIGN.md §9c.
//
// A record stores no decoded size, and the decoded size is not the block size (the FCX7 early
// stop, the FCX8 tail-zero rule), so seeking needs the decoders' own size computation:
//
//   size pass      per codec (dec7_sizes in fcx_dec.hip, lz78_sizes in fcx_lz78_dec.hip): the record
//                  walk and the stages up to the decoded sizes, nothing expanded;
//   k_rindex       one workgroup: rec_off from the walk, dec_off = exclusive scan of the sizes;
//   k_rlocate      one thread: total, the clamped range and the first and last record it touches
//                  (two binary searches over dec_off; records of decoded size 0 fall out of them);
//   clipped decode per codec (dec7_range, lz78_range) on the sub-run of those records: the decode
//                  stages as in a full decode, each record's size checked against the index, and
//                  an expansion that stores only the bytes of the window, at d_out[0 ..).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "fcx.h"
#include "fcx_dec_shared.h"

namespace fcx {

// what k_rlocate leaves for the host (u64 each); kRwTotal is also k_rindex's
constexpr uint32_t kRwTotal = 0, kRwOutLen = 1, kRwFirst = 2, kRwLast = 3, kRwRecOff = 4, kRwDecOff = 5, kRwWords = 8;

// rec_off[k] = offset of record k's length prefix, rec_off[n] = the bytes the records span;
// dec_off = exclusive scan of the decoded sizes, dec_off[n] = their total (also words[kRwTotal])
__global__ __launch_bounds__(1024) void k_rindex(uint32_t n, const uint64_t *roff, const uint32_t *rlen,
                                                 const uint32_t *dsize, uint64_t *rec_off, uint64_t *dec_off,
                                                 uint64_t *words) {
    __shared__ uint64_t sh[16];
    __shared__ uint64_t carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n; b0 += 1024) {
        const uint32_t b = b0 + tid;
        const uint64_t v = b < n ? dsize[b] : 0;
        uint64_t inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t t = __shfl_up(inc, o, 64);
            if (lane >= (uint32_t)o) inc += t;
        }
        if (lane == 63) sh[wv] = inc;
        __syncthreads();
        uint64_t pre = carry + inc - v, all = 0;
        for (uint32_t w = 0; w < 16; w++) {
            if (w < wv) pre += sh[w];
            all += sh[w];
        }
        if (b < n) {
            dec_off[b] = pre;
            rec_off[b] = roff[b] - 4;
            if (b + 1 == n) rec_off[n] = roff[b] + rlen[b];
        }
        __syncthreads();
        if (tid == 0) carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        dec_off[n] = carry;
        words[kRwTotal] = carry;
    }
}

// the last k in [0, n) with dec_off[k] <= x when dec_off ascends (x < dec_off[n]); always in [0, n)
__device__ inline uint32_t rec_of(const uint64_t *dec_off, uint32_t n, uint64_t x) {
    uint32_t lo = 1, hi = n;   // the first k in [1, n] with dec_off[k] > x (n if none)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (dec_off[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

// one thread: the range clamped to the run and the records it touches.  A record of decoded size 0
// has dec_off[k] == dec_off[k + 1] and is never the answer of rec_of, so the sub-run starts and
// ends with a record that has bytes in the range.
__global__ void k_rlocate(uint32_t n, const uint64_t *rec_off, const uint64_t *dec_off, uint64_t off, uint64_t len,
                          uint64_t *words) {
    const uint64_t total = dec_off[n];
    const uint64_t lo = off < total ? off : total, cnt = len < total - lo ? len : total - lo;
    words[kRwTotal] = total;
    words[kRwOutLen] = cnt;
    if (cnt == 0) return;
    const uint32_t first = rec_of(dec_off, n, lo);
    uint32_t last = rec_of(dec_off, n, lo + cnt - 1);
    if (last < first) last = first;   // (an index that does not ascend)
    words[kRwFirst] = first;
    words[kRwLast] = last;
    words[kRwRecOff] = rec_off[first];
    words[kRwDecOff] = dec_off[first];
}

static int range_words(RangeScratch &R) {
    if (!R.host_words) {
        FCX_TRY(R.words.reserve(8 * kRwWords, "range words"));
        FCX_HIP(R.host_words.alloc(8 * kRwWords));
    }
    return FCX_OK;
}

static bool kind_ok(char kind) { return kind == '7' || kind == '8'; }

// fcx_index_shard behind its argument checks (nblocks > 0)
static int index_run(fcx_dctx *c, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint64_t *d_rec_off,
                     uint64_t *d_dec_off, uint64_t *total, hipStream_t st) {
    RangeScratch &R = c->rg;
    FCX_TRY(range_words(R));
    FCX_TRY(R.roff.reserve(8ull * nblocks, "record offsets"));
    FCX_TRY(R.rlen.reserve(4ull * nblocks, "record lengths"));
    FCX_TRY(R.dsize.reserve(4ull * nblocks, "decoded sizes"));
    if (kind == '7') FCX_TRY(dec7_sizes(c, d_in, in_len, nblocks, R.roff, R.rlen, R.dsize, st));
    else FCX_TRY(lz78_sizes(c, d_in, in_len, nblocks, R.roff, R.rlen, R.dsize, st));
    hipLaunchKernelGGL(k_rindex, dim3(1), dim3(1024), 0, st, nblocks, R.roff, R.rlen, R.dsize, d_rec_off, d_dec_off, R.words);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(R.host_words, R.words, 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    R.stats[0] = nblocks;
    if (total) *total = R.host_words[kRwTotal];
    return FCX_OK;
}

int range_shard(fcx_dctx *c, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, const uint64_t *d_rec_off,
                const uint64_t *d_dec_off, uint64_t off, uint64_t len, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                hipStream_t st, uint64_t rec_base, uint64_t *total) {
    FCX_HIP(hipSetDevice(c->device));
    RangeScratch &R = c->rg;
    c->times.reset();
    memset(R.stats, 0, sizeof(R.stats));
    *out_len = 0;
    if (total) *total = 0;
    if (nblocks == 0) return FCX_OK;
    FCX_TRY(range_words(R));
    if (!d_rec_off) {   // the call's own index, in the context's scratch
        FCX_TRY(R.rec_off.reserve(8ull * nblocks + 8, "index"));
        FCX_TRY(R.dec_off.reserve(8ull * nblocks + 8, "index"));
        FCX_TRY(index_run(c, kind, d_in, in_len, nblocks, R.rec_off, R.dec_off, nullptr, st));
        d_rec_off = R.rec_off;
        d_dec_off = R.dec_off;
        R.stats[3] = 1;
    }
    hipLaunchKernelGGL(k_rlocate, dim3(1), dim3(1), 0, st, nblocks, d_rec_off, d_dec_off, off, len, R.words);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(R.host_words, R.words, 8 * kRwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    const uint64_t *hw = R.host_words;
    const uint64_t n_out = hw[kRwOutLen];
    if (total) *total = hw[kRwTotal];
    *out_len = n_out;
    if (n_out > cap) return fail(FCX_ERR_CAPACITY, "fcx_decompress_range_shard: output capacity too small");
    if (n_out == 0) return FCX_OK;
    if (!d_out) return fail(FCX_ERR_ARG, "fcx_decompress_range_shard: NULL d_out");
    const uint64_t first = hw[kRwFirst], last = hw[kRwLast], ro = hw[kRwRecOff], d0 = hw[kRwDecOff];
    // (only a caller's index can fail these: where it points must be inside the run)
    if (ro > in_len || in_len - ro < 4 || d0 > off)
        return fail(FCX_ERR_FORMAT, "the index disagrees with the run: record " + std::to_string(rec_base + first + 1) +
                                        " is not where it says");
    const uint32_t nrec = (uint32_t)(last - first + 1);
    const DClip w{off - d0, off - d0 + n_out};
    uint64_t stored = 0;
    R.stats[1] = nrec;
    if (kind == '7') FCX_TRY(dec7_range(c, d_in + ro, in_len - ro, nrec, d_dec_off + first, w, d_out, st, &stored));
    else FCX_TRY(lz78_range(c, d_in + ro, in_len - ro, nrec, d_dec_off + first, w, d_out, st, rec_base + first, &stored));
    R.stats[2] = stored;
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_index_shard(fcx_dctx *c, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint64_t *d_rec_off,
                    uint64_t *d_dec_off, uint64_t *total, void *stream) {
    if (!c || !d_rec_off || !d_dec_off || (!d_in && (in_len || nblocks)))
        return fail(FCX_ERR_ARG, "fcx_index_shard: NULL argument");
    if (!kind_ok(kind)) return fail(FCX_ERR_ARG, "fcx_index_shard: kind must be '7' or '8'");
    hipStream_t st = (hipStream_t)stream;
    FCX_HIP(hipSetDevice(c->device));
    c->times.reset();
    memset(c->rg.stats, 0, sizeof(c->rg.stats));
    if (total) *total = 0;
    if (nblocks == 0) {   // rec_off[0] = dec_off[0] = 0
        FCX_HIP(hipMemsetAsync(d_rec_off, 0, 8, st));
        FCX_HIP(hipMemsetAsync(d_dec_off, 0, 8, st));
        FCX_HIP(hipStreamSynchronize(st));
        return FCX_OK;
    }
    return index_run(c, kind, d_in, in_len, nblocks, d_rec_off, d_dec_off, total, st);
}

int fcx_decompress_range_shard(fcx_dctx *c, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks,
                               const uint64_t *d_rec_off, const uint64_t *d_dec_off, uint64_t off, uint64_t len,
                               uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream) {
    if (!c || !out_len || (!d_in && (in_len || nblocks)))
        return fail(FCX_ERR_ARG, "fcx_decompress_range_shard: NULL argument");
    if (!kind_ok(kind)) return fail(FCX_ERR_ARG, "fcx_decompress_range_shard: kind must be '7' or '8'");
    if (!d_rec_off != !d_dec_off) return fail(FCX_ERR_ARG, "fcx_decompress_range_shard: half an index (one pointer NULL)");
    return range_shard(c, kind, d_in, in_len, nblocks, d_rec_off, d_dec_off, off, len, d_out, cap, out_len,
                       (hipStream_t)stream, 0, nullptr);
}

int fcx_dctx_range_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_range_stats: bad argument");
    for (int i = 0; i < n && i < FCX_RANGE_STATS; i++) out[i] = c->rg.stats[i];
    return FCX_OK;
}

}  // extern "C"
