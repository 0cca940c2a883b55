// fcx_digest.hip — content digests (gfx950): the CRC-32 (zlib's) of many byte segments of a device
// buffer, fcx_digest_shard and fcx_check_shard of include/fcx.h (their stream and host forms: fcx_stream.hip).
// DESIGN.md §9f.
//
// gfx950 has no carry-less multiply, so the sum is table-driven, and a segment is not one lane's walk:
//
//   k_dgcrc      workgroup (segment x chunk of 64 KiB).  The chunk is 16-byte pieces, right-aligned on a
//                grid of 16 rows x 256 lanes: lane t takes the piece of column t in every row, so a row
//                is 4 KiB of neighbouring loads.  A lane keeps the pure remainder (init and xorout 0) of
//                its pieces: a row further it is folded over the 4080 bytes between its pieces (4 table
//                reads) and the next piece goes in by slicing (16 table reads); both tables sit in LDS.
//                Then lane t multiplies by x^(8 * 16 * (255 - t)), its distance to the chunk's end, the
//                256 products are XORed (shuffles, 4 words of LDS), and one lane adds the chunk's last
//                < 16 bytes, multiplies by x^(8 * bytes behind the chunk in its segment), folds in init
//                and xorout from the segment's length (chunk 0 only) and XORs the word into the
//                segment's with one atomic.  XOR commutes: no order among workgroups matters.
//   reads        16 bytes through ld16_bounded (fcx_ld16.h), as k_vcompare and k_rplan do: nothing outside a
//                segment is read.
//   segments     three forms of one kernel: strided (block k at k B, the last ragged to n), a u64 offsets
//                array (the run's dec_off), and a list of device addresses and lengths (a check's
//                decoded prefixes and RAW bytes).
//   a check      the run core: index, the entry map of fcx_repair.hip, then per record group
//                the decode into the verification's bounded buffer, k_dgplan (per record its two
//                segments), k_dgcrc; at the end k_dgsummary: a repaired block's CRC-32 combined from its
//                parts, the compare with the expected values, the totals.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_crc32.h"
#include "fcx_dec_shared.h"
#include "fcx_ld16.h"

namespace fcx {

constexpr uint32_t kDgThreads = 256;
constexpr uint32_t kDgRows = 16;                          // 16-byte pieces per lane and chunk
constexpr uint32_t kDgRowBytes = 16 * kDgThreads;         // 4 KiB
constexpr uint32_t kDgPieces = kDgRows * kDgThreads;
constexpr uint32_t kDgChunk = kDgRows * kDgRowBytes;      // bytes of a segment one workgroup sums (64 KiB)
constexpr uint32_t kDgSlice = 4;                          // bytes per slicing round by default: 4 tables in LDS
constexpr uint64_t kDgMaxGrid = 0x7FFFFFFFull;
// the tables, u32 each: 16 slicing tables (T[0] the byte table), the fold over a row less a piece, a
// lane's distance to the chunk's end, x^(8 b 2^(8k)) for the four bytes b of a length
constexpr uint32_t kDgtSlice = 0, kDgtFold = 16 * 256, kDgtLane = kDgtFold + 4 * 256, kDgtPow = kDgtLane + 256,
                   kDgtWords = kDgtPow + 4 * 256;
constexpr uint32_t kGfOne = 0x80000000u, kGfX8 = 0x00800000u, kGfPoly = 0xEDB88320u;

enum { kDgStrided = 0, kDgOffsets = 1, kDgList = 2 };

// a b mod P (reflected: bit 31 is x^0)
__device__ inline uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        p ^= b & (uint32_t)(-(int32_t)((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kGfPoly & (uint32_t)(-(int32_t)(b & 1u)));
    }
    return p;
}

// x^(8m) mod P from the power tables: at most three multiplies
__device__ inline uint32_t gf_xpow8(const uint32_t *__restrict__ tables, uint32_t m) {
    uint32_t x = kGfOne;
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t b = (m >> (8 * k)) & 0xFFu;
        if (b) x = x == kGfOne ? tables[kDgtPow + 256 * k + b] : gf_mul(x, tables[kDgtPow + 256 * k + b]);
    }
    return x;
}

// what init and xorout add to the pure remainder of len bytes
__device__ inline uint32_t crc_init_term(uint32_t xlen) { return gf_mul(0xFFFFFFFFu, xlen) ^ 0xFFFFFFFFu; }

// the CRC-32 of len copies of v, without memory: doubling over the bits of len
__device__ inline uint32_t crc_fill(const uint32_t *__restrict__ tables, uint32_t v, uint32_t len) {
    uint32_t r = 0, x = kGfOne;   // the pure remainder of the m copies so far, x^(8m)
    for (int b = 31 - (len ? __builtin_clz(len) : 31); b >= 0; b--) {
        r = gf_mul(r, x) ^ r;
        x = gf_mul(x, x);
        if ((len >> b) & 1u) {
            r = tables[kDgtSlice + ((r ^ v) & 0xFFu)] ^ (r >> 8);
            x = gf_mul(x, kGfX8);
        }
    }
    return r ^ crc_init_term(x);
}

// N bytes (the words x[0, N / 4), the state already in x[0]) through the slicing tables
template <int N>
__device__ inline uint32_t crc_round(const uint32_t *sT, const uint32_t *x) {
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < N / 4; j++)
#pragma unroll
        for (int b = 0; b < 4; b++) r ^= sT[256 * (N - 1 - (4 * j + b)) + ((x[j] >> (8 * b)) & 0xFFu)];
    return r;
}

// The CRC-32 of segments of a device buffer, XORed into crc[seg] (zeroed before; an empty segment stays
// 0).  Workgroup (chunk c of segment seg0 + blockIdx.x / cps).  Segment k: FORM kDgStrided
// [k B, min(n, (k + 1) B)) of data; kDgOffsets [off[k], off[k + 1]) less off_base of data; kDgList lens[k]
// bytes at the device address off[k].  N: the bytes of a slicing round.
template <int FORM, int N>
__global__ __launch_bounds__(kDgThreads) void k_dgcrc(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off,
                                                      uint64_t off_base, const uint32_t *__restrict__ lens, uint64_t n,
                                                      uint32_t B, uint32_t seg0, uint32_t cps,
                                                      const uint32_t *__restrict__ tables, uint32_t *__restrict__ crc) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[256 * N], sF[256 * 4];
    __shared__ uint32_t sR[kDgThreads / 64];
    const uint32_t seg = seg0 + blockIdx.x / cps, c = blockIdx.x % cps, t = threadIdx.x;
    const uint8_t *p;
    uint32_t len;
    if (FORM == kDgStrided) {
        len = block_len(seg, n, B);
        p = data + (uint64_t)seg * B;
    } else if (FORM == kDgOffsets) {
        const uint64_t a = off[seg];
        len = (uint32_t)(off[seg + 1] - a);
        p = data + (a - off_base);
    } else {
        len = lens[seg];
        p = (const uint8_t *)(uintptr_t)off[seg];
    }
    if ((uint64_t)c * kDgChunk >= len) return;   // (the whole workgroup; an empty segment has no chunk)
    for (uint32_t i = t; i < 64 * N; i += kDgThreads) ((uint4 *)sT)[i] = ((const uint4 *)(tables + kDgtSlice))[i];
    ((uint4 *)sF)[t] = ((const uint4 *)(tables + kDgtFold))[t];
    __syncthreads();
    const uint32_t c0 = c * kDgChunk, clen = min(kDgChunk, len - c0);
    const uint32_t nfull = clen >> 4, skip = kDgPieces - nfull;   // whole pieces, right-aligned on the grid
    const uint32_t sh = (uint32_t)((uintptr_t)p & 15);            // (c0 is a multiple of 16: one shift for all pieces)
    uint32_t r = 0;
#pragma unroll 4
    for (uint32_t s = 0; s < kDgRows; s++) {
        const uint32_t v = s * kDgThreads + t;
        if (v < skip) continue;
        const uint32_t i = c0 + 16 * (v - skip);
        const uint4 w = ld16_bounded(p, i, sh, len);
        uint32_t x[4] = {w.x, w.y, w.z, w.w};
        // the remainder so far, kDgRowBytes further: folded over all but the piece's 16 bytes, which the
        // slicing rounds then cross with the piece
        r = sF[r & 0xFFu] ^ sF[256 + ((r >> 8) & 0xFFu)] ^ sF[512 + ((r >> 16) & 0xFFu)] ^ sF[768 + (r >> 24)];
#pragma unroll
        for (int q = 0; q < 16 / N; q++) {
            x[q * (N / 4)] ^= r;
            r = crc_round<N>(sT, x + q * (N / 4));
        }
    }
    r = gf_mul(r, tables[kDgtLane + t]);   // to the end of the chunk's whole pieces
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o, 64);
    if ((t & 63) == 0) sR[t >> 6] = r;
    __syncthreads();
    if (t != 0) return;
    r = sR[0] ^ sR[1] ^ sR[2] ^ sR[3];
    for (uint32_t i = c0 + 16 * nfull; i < c0 + clen; i++) r = sT[(r ^ p[i]) & 0xFFu] ^ (r >> 8);
    const uint32_t behind = len - c0 - clen;
    if (behind) r = gf_mul(r, gf_xpow8(tables, behind));
    if (c == 0) r ^= crc_init_term(gf_xpow8(tables, len));
    atomicXor(crc + seg, r);
}

// One thread per record of the group [k0, k0 + nrec), decoded back to back at dec (gbytes bytes; byte 0
// is decoded offset dec_base of the run): its two segments.  2k: the decoded record, or below an entry's
// `from` only; 2k + 1: a RAW entry's bytes.  The entries passed k_rmap, and still nothing they say moves
// a segment out of dec[0, gbytes) or data[0, data_bytes).
__global__ __launch_bounds__(kDgThreads) void k_dgplan(const uint8_t *__restrict__ dec, uint64_t dec_base, uint64_t gbytes,
                                                       const uint64_t *__restrict__ dec_off, uint32_t k0, uint32_t nrec,
                                                       const uint32_t *__restrict__ entry_of,
                                                       const fcx_repair_entry *__restrict__ entries,
                                                       const uint8_t *__restrict__ data, uint64_t data_bytes,
                                                       uint64_t *__restrict__ seg_at, uint32_t *__restrict__ seg_len) {
    const uint32_t j = blockIdx.x * kDgThreads + threadIdx.x;
    if (j >= nrec) return;
    const uint32_t k = k0 + j;
    const uint64_t d0 = min(dec_off[k] - dec_base, gbytes);
    uint32_t keep = (uint32_t)min(dec_off[k + 1] - dec_off[k], gbytes - d0), raw = 0;
    uint64_t raw_at = 0;
    const uint32_t ei = entry_of[k];
    if (ei != kNoEntry) {
        const fcx_repair_entry e = entries[ei];
        keep = min(keep, e.from);
        if (e.kind == FCX_REPAIR_RAW && e.data_off <= data_bytes && e.len <= data_bytes - e.data_off) {
            raw = e.len;
            raw_at = (uint64_t)(uintptr_t)(data + e.data_off);
        }
    }
    seg_at[2 * k] = (uint64_t)(uintptr_t)(dec + d0);
    seg_len[2 * k] = keep;
    seg_at[2 * k + 1] = raw_at;
    seg_len[2 * k + 1] = raw;
}

// One workgroup over the nblocks records: the block record k gives (its decoded bytes, part[k] with
// pstride 1; with a repair, pstride 2, the kept prefix part[2k] and for an entry its bytes part[2k + 1]:
// the CRC-32 combined from the parts, a fill's computed), its
// length and CRC-32 to blocks (may be null), the compare with block k of the ncrc expected ones (a
// record from ncrc on fails), and the totals into the status words (zeroed before, kVwFirst preset to ~0).
__global__ __launch_bounds__(1024) void k_dgsummary(uint32_t nblocks, uint32_t ncrc, const uint64_t *__restrict__ dec_off,
                                                    uint64_t n, uint32_t B, const uint32_t *__restrict__ entry_of,
                                                    const fcx_repair_entry *__restrict__ entries,
                                                    const uint32_t *__restrict__ part, uint32_t pstride,
                                                    const uint32_t *__restrict__ want,
                                                    const uint32_t *__restrict__ tables, uint32_t *__restrict__ blocks,
                                                    uint64_t *__restrict__ words) {
    uint64_t failing = 0, first = ~0ull, sized = 0, bytes = 0;
    for (uint32_t k = threadIdx.x; k < nblocks; k += 1024) {
        const uint32_t blen = k < ncrc ? block_len(k, n, B) : 0u;
        uint32_t rlen = (uint32_t)(dec_off[k + 1] - dec_off[k]), c = part[pstride * k];
        const uint32_t ei = entry_of[k];
        if (ei != kNoEntry) {
            const fcx_repair_entry e = entries[ei];
            const uint32_t tail = e.kind == FCX_REPAIR_FILL ? crc_fill(tables, e.fill & 0xFFu, e.len) : part[2 * k + 1];
            c = gf_mul(c, gf_xpow8(tables, e.len)) ^ tail;
            rlen = e.from + e.len;
        }
        if (blocks) {
            blocks[2 * k] = rlen;
            blocks[2 * k + 1] = c;
        }
        if (rlen != blen) sized++;
        if (k >= ncrc || rlen != blen || c != want[k]) {
            failing++;
            bytes += blen;
            first = min(first, (uint64_t)k);
        }
    }
    publish_verdict(failing, first, sized, bytes, nblocks, dec_off, words);
}

namespace {
const char *kDgStageNames[] = {"index", "decode", "digest", "summary"};
constexpr int kDgStages = 4;

// the tables of k_dgcrc, from the host mirror
std::vector<uint32_t> make_tables() {
    std::vector<uint32_t> t(kDgtWords);
    const uint32_t *t0 = fcx_crc::table();
    for (uint32_t i = 0; i < 256; i++) t[kDgtSlice + i] = t0[i];
    for (uint32_t k = 1; k < 16; k++)
        for (uint32_t i = 0; i < 256; i++) {
            const uint32_t v = t[kDgtSlice + 256 * (k - 1) + i];
            t[kDgtSlice + 256 * k + i] = (v >> 8) ^ t0[v & 0xFFu];
        }
    const uint32_t fold = fcx_crc::xpow8(kDgRowBytes - 16);
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t b = 0; b < 256; b++) {
            t[kDgtFold + 256 * k + b] = fcx_crc::mul(b << (8 * k), fold);
            t[kDgtPow + 256 * k + b] = fcx_crc::xpow8((uint64_t)b << (8 * k));
        }
    for (uint32_t l = 0; l < kDgThreads; l++) t[kDgtLane + l] = fcx_crc::xpow8(16ull * (kDgThreads - 1 - l));
    return t;
}

int ready(fcx_dctx *c, hipStream_t st) {
    DigestScratch &D = c->dg;
    if (!D.host_words) {
        FCX_TRY(D.words.reserve(8 * kDgwWords, "digest words"));
        FCX_HIP(D.host_words.alloc(8 * kDgwWords));
    }
    if (!D.tables) {
        const std::vector<uint32_t> t = make_tables();
        FCX_TRY(D.tables.reserve(4ull * kDgtWords, "digest tables"));
        FCX_HIP(hipMemcpyAsync(D.tables, t.data(), 4ull * kDgtWords, hipMemcpyHostToDevice, st));
        FCX_HIP(hipStreamSynchronize(st));   // (t goes with this frame)
    }
    for (uint64_t &v : D.stats) v = 0;
    return FCX_OK;
}

// k_dgcrc over nseg segments of at most max_len bytes, crc[0, nseg) zeroed first; as many launches as
// the grid limit asks for
template <int FORM>
int launch_crc(fcx_dctx *c, const uint8_t *data, const uint64_t *off, uint64_t off_base, const uint32_t *lens, uint64_t n,
               uint32_t B, uint32_t nseg, uint64_t max_len, uint32_t *crc, hipStream_t st) {
    if (nseg == 0) return FCX_OK;
    FCX_HIP(hipMemsetAsync(crc, 0, 4ull * nseg, st));
    const uint32_t cps = (uint32_t)((max_len + kDgChunk - 1) / kDgChunk);
    if (cps == 0) return FCX_OK;
    const uint32_t per = (uint32_t)std::min<uint64_t>(nseg, kDgMaxGrid / cps);
    for (uint32_t s0 = 0; s0 < nseg; s0 += per) {
        const uint32_t ns = std::min(per, nseg - s0);
        auto *kernel = c->dg.slice == 16 ? k_dgcrc<FORM, 16> : c->dg.slice == 8 ? k_dgcrc<FORM, 8> : k_dgcrc<FORM, kDgSlice>;
        hipLaunchKernelGGL(kernel, dim3(ns * cps), dim3(kDgThreads), 0, st, data, off, off_base, lens, n, B, s0, cps,
                           (const uint32_t *)c->dg.tables, crc);
    }
    FCX_HIP(hipGetLastError());
    return FCX_OK;
}
}  // namespace

int digest_run(fcx_dctx *c, const uint8_t *d_data, uint64_t n, uint32_t B, uint32_t *d_crc, uint32_t *whole, hipStream_t st) {
    if (whole) *whole = 0;
    if (n == 0) {
        for (uint64_t &v : c->dg.stats) v = 0;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c, st));
    const uint32_t nb = (uint32_t)((n + B - 1) / B);
    FCX_TRY(launch_crc<kDgStrided>(c, d_data, nullptr, 0, nullptr, n, B, nb, std::min<uint64_t>(n, B), d_crc, st));
    c->dg.stats[0] = nb;
    c->dg.stats[1] = n;
    if (!whole) return FCX_OK;
    std::vector<uint32_t> v(nb);
    FCX_HIP(hipMemcpyAsync(v.data(), d_crc, 4ull * nb, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    const uint32_t xb = fcx_crc::xpow8(B);   // every block but the last is B bytes
    uint32_t all = 0;
    for (uint32_t k = 0; k + 1 < nb; k++) all = fcx_crc::mul(all, xb) ^ v[k];
    *whole = fcx_crc::combine(all, v[nb - 1], n - (uint64_t)(nb - 1) * B);
    return FCX_OK;
}

int check_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint32_t ncrc, uint64_t n,
              uint32_t B, const fcx_repair_entry *d_entries, uint32_t nentries, const uint8_t *d_data, uint64_t data_bytes,
              const uint32_t *d_crc, uint32_t *d_blocks, uint64_t *stats, hipStream_t st, uint64_t rec_base) {
    for (int i = 0; i < FCX_VERIFY_STATS; i++) stats[i] = 0;
    stats[kVwFirst] = ~0ull;
    if (nblocks == 0) {
        for (uint64_t &v : c->dg.stats) v = 0;
        return FCX_OK;
    }
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c, st));
    DigestScratch &D = c->dg;
    RepairScratch &P = c->rp;
    VerifyScratch &V = c->vf;
    RangeScratch &R = c->rg;
    RunTimes T(c, kDgStages, st);
    RunIndex ix;
    FCX_TRY(D.seg_at.reserve(16ull * nblocks, "digest segments"));
    FCX_TRY(D.seg_len.reserve(8ull * nblocks, "digest segments"));
    FCX_TRY(D.part.reserve(8ull * nblocks, "digest parts"));
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    FCX_TRY(T.add(0, 1));
    const std::vector<uint64_t> &doff = ix.doff;
    // the entries against the index, as an apply checks them
    FCX_TRY(launch_entry_map(c, d_entries, nentries, nblocks, n, B, data_bytes, false, st));
    FCX_HIP(hipMemsetAsync(D.words, 0, 8 * kDgwWords, st));
    FCX_HIP(hipMemsetAsync(D.words + kVwFirst, 0xFF, 8, st));
    FCX_HIP(hipMemsetAsync(D.part, 0, 8ull * nblocks, st));
    FCX_HIP(hipStreamSynchronize(st));
    FCX_TRY(entry_map_result(c, rec_base));
    std::vector<RunGroup> groups;
    FCX_TRY(run_groups(c, ix, nblocks, &groups));
    for (const RunGroup &g : groups) {
        const uint32_t g0 = g.g0, nrec = g.g1 - g0;
        uint64_t longest = nentries ? B : 0;
        for (uint32_t k = g0; k < g.g1; k++) longest = std::max(longest, doff[k + 1] - doff[k]);
        T.mark(1);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g0, nrec, V.buf, g.gbytes, st, rec_base, "fcx_check_shard"));
        T.mark(2);
        if (nentries == 0) {   // the records as they are: the index's offsets are the segments
            FCX_TRY(launch_crc<kDgOffsets>(c, V.buf, R.dec_off + g0, doff[g0], nullptr, 0, 0, nrec, longest, D.part + g0, st));
        } else {
            hipLaunchKernelGGL(k_dgplan, dim3((nrec + kDgThreads - 1) / kDgThreads), dim3(kDgThreads), 0, st, V.buf, doff[g0],
                               g.gbytes, R.dec_off, g0, nrec, P.entry_of, d_entries, d_data, data_bytes, D.seg_at, D.seg_len);
            FCX_TRY(launch_crc<kDgList>(c, nullptr, D.seg_at + 2ull * g0, 0, D.seg_len + 2ull * g0, 0, 0, 2 * nrec, longest,
                                        D.part + 2ull * g0, st));
        }
        T.mark(3);
        FCX_TRY(T.add(1, 3));
        D.stats[0] += nentries ? 2ull * nrec : nrec;
        D.stats[2]++;
    }
    T.mark(3);
    hipLaunchKernelGGL(k_dgsummary, dim3(1), dim3(1024), 0, st, nblocks, ncrc, R.dec_off, n, B, P.entry_of, d_entries, D.part,
                       nentries ? 2u : 1u, d_crc, (const uint32_t *)D.tables, d_blocks, D.words);
    T.mark(4);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(D.host_words, D.words, 8 * kDgwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < FCX_VERIFY_STATS; i++) stats[i] = D.host_words[i];
    D.stats[1] = doff[nblocks] + data_bytes;   // (at most: what is kept of a repaired record is a prefix)
    D.stats[3] = nentries;
    FCX_TRY(T.add(3, 4));
    T.publish(c, kDgStageNames, kDgStages);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_digest_shard(fcx_dctx *c, const uint8_t *d_data, uint64_t n, uint32_t block_bytes, uint32_t *d_crc, uint32_t *whole,
                     void *stream) {
    if (!c || (n && (!d_data || !d_crc))) return fail(FCX_ERR_ARG, "fcx_digest_shard: NULL argument");
    if (block_bytes == 0 || block_bytes > FCX_MAX_BLOCK_BYTES)
        return fail(FCX_ERR_ARG, "fcx_digest_shard: block_bytes outside [1, FCX_MAX_BLOCK_BYTES]");
    if ((n + block_bytes - 1) / block_bytes > kDgMaxGrid) return fail(FCX_ERR_ARG, "fcx_digest_shard: too many blocks for one call");
    return digest_run(c, d_data, n, block_bytes, d_crc, whole, (hipStream_t)stream);
}

int fcx_digest_segments(fcx_dctx *c, const uint8_t *d_data, const uint64_t *d_off, uint32_t nseg, uint32_t *d_crc,
                        void *stream) {
    if (!c || (nseg && (!d_data || !d_off || !d_crc))) return fail(FCX_ERR_ARG, "fcx_digest_segments: NULL argument");
    for (uint64_t &v : c->dg.stats) v = 0;
    if (nseg == 0) return FCX_OK;
    hipStream_t st = (hipStream_t)stream;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c, st));
    // the offsets on the host: they must ascend, and the longest segment sizes the grid
    std::vector<uint64_t> off((uint64_t)nseg + 1);
    FCX_HIP(hipMemcpyAsync(off.data(), d_off, 8ull * nseg + 8, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    uint64_t longest = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        if (off[k + 1] < off[k] || off[k + 1] - off[k] > 0xFFFFFFFFull)
            return fail(FCX_ERR_ARG, "fcx_digest_segments: offsets must ascend, a segment is shorter than 2^32 bytes");
        longest = std::max(longest, off[k + 1] - off[k]);
    }
    FCX_TRY(launch_crc<kDgOffsets>(c, d_data, d_off, 0, nullptr, 0, 0, nseg, longest, d_crc, st));
    c->dg.stats[0] = nseg;
    c->dg.stats[1] = off[nseg] - off[0];
    return FCX_OK;
}

uint32_t fcx_crc32(uint32_t crc, const uint8_t *p, uint64_t n) { return p ? fcx_crc::crc32(crc, p, n) : crc; }
uint32_t fcx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return fcx_crc::combine(crc_a, crc_b, len_b); }

int fcx_check_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint64_t n,
                    uint32_t block_bytes, const fcx_repair_entry *d_entries, uint32_t nentries, const uint8_t *d_data,
                    uint64_t data_bytes, const uint32_t *d_crc, uint32_t *d_blocks, uint64_t *stats, void *stream) {
    if (!stats) return fail(FCX_ERR_ARG, "fcx_check_shard: NULL argument");
    FCX_TRY(run_args("fcx_check_shard", c, kind, d_rec, nblocks, n, block_bytes));
    if ((nblocks && !d_crc) || (nentries && !d_entries) || (data_bytes && !d_data))
        return fail(FCX_ERR_ARG, "fcx_check_shard: NULL argument");
    return check_run(c, kind, d_rec, rec_len, nblocks, nblocks, n, block_bytes, d_entries, nentries, d_data, data_bytes, d_crc,
                     d_blocks, stats, (hipStream_t)stream, 0);
}

int fcx_dctx_digest_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_digest_stats: bad argument");
    for (int i = 0; i < n && i < FCX_DIGEST_STATS; i++) out[i] = c->dg.stats[i];
    return FCX_OK;
}

int fcx_dctx_set_digest_slice(fcx_dctx *c, uint32_t bytes) {
    if (!c || (bytes != 0 && bytes != 4 && bytes != 8 && bytes != 16)) return fail(FCX_ERR_ARG, "fcx_dctx_set_digest_slice: bad argument");
    c->dg.slice = bytes ? bytes : kDgSlice;
    return FCX_OK;
}

}  // extern "C"
