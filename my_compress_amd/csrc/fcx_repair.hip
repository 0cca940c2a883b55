// fcx_repair.hip — the repair of a device-resident run of FCX7 / FCX8 records (gfx950):
// fcx_repair_build_shard and fcx_repair_apply_shard of include/fcx.h.  DESIGN.md §9e.
//
// The records are the reference's bytes and its decoder does not return every input (fcx_verify.hip),
// so what is lost is kept beside them: one entry per block that does not come back.
//
//   build   verify_run (index, grouped decode, k_vcompare, k_vsummary: the pairs), then
//     k_rplan    one workgroup per differing record: is the block's suffix behind the first
//                difference one byte value (FILL) or not (RAW)?
//     k_rscan    one workgroup: the entries compacted in block order, the exclusive u64 sum of the
//                RAW lengths as data_off, the counts into the status words;
//     k_rgather  (entry x 16 KiB chunk): a RAW suffix of the original to d_data + data_off.
//   apply   the index, then the entry map (launch_entry_map, which a check of fcx_digest.hip calls too)
//     k_rmap     one thread per entry: the checks of fcx.h against the index, entry_of[block];
//     k_rcheck   one thread per record: a record without an entry decodes to its block's length;
//     the decode: a group of records without entries straight to its place in d_out, a group with
//     entries into the verification's bounded buffer, and
//     k_rapply   (record x 16 KiB chunk): the decoded prefix, then the RAW bytes or the fill byte.
//
// Both copies store 16 aligned bytes per lane on the destination and read the source, which sits
// anywhere, through ld16_bounded (fcx_ld16.h).  The host half of an apply is the run core's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"
#include "fcx_device.h"   // wave_sum_u64
#include "fcx_ld16.h"

namespace fcx {

static_assert(sizeof(fcx_repair_entry) == 32, "the entry is 32 bytes on the device and in the file");

constexpr uint32_t kRThreads = 256;
constexpr uint32_t kRChunk = 16384;                    // bytes of a block one workgroup copies
constexpr uint32_t kRRound = 16 * kRThreads * 16;      // bytes k_rplan tests between two votes (64 KiB)
constexpr uint64_t kRMaxGrid = 0x7FFFFFFFull;

// cnt bytes from src to dst by the workgroup, both anywhere.  Head (to the destination's next 16-byte
// boundary) and tail go byte by byte; in between every lane stores 16 aligned bytes, read by ld16_bounded
// within [rlo, rhi), so nothing outside [rlo, rhi) is read and nothing outside [dst, dst + cnt) is written.
__device__ inline void copy_aligned(uint8_t *dst, const uint8_t *src, uint32_t cnt, const uint8_t *rlo, const uint8_t *rhi) {
    const uint32_t t = threadIdx.x;
    const uint32_t head = min(cnt, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if (t < head) dst[t] = src[t];
    const uint32_t body = (cnt - head) & ~15u;
    uint8_t *d = dst + head;
    const uint8_t *s = src + head;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 15);
    const uint64_t s0 = (uint64_t)(s - rlo), rlen = (uint64_t)(rhi - rlo);
    for (uint32_t i = 16 * t; i < body; i += 16 * kRThreads) *(uint4 *)(d + i) = ld16_bounded(rlo, s0 + i, sh, rlen);
    const uint32_t tail = cnt - head - body;   // < 16
    if (t < tail) d[body + t] = s[body + t];
}

// the same stores with one byte value
__device__ inline void fill_aligned(uint8_t *dst, uint32_t cnt, uint32_t v) {
    const uint32_t t = threadIdx.x;
    const uint32_t head = min(cnt, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if (t < head) dst[t] = (uint8_t)v;
    const uint32_t body = (cnt - head) & ~15u, vv = (v & 0xFFu) * 0x01010101u;
    uint8_t *d = dst + head;
    for (uint32_t i = 16 * t; i < body; i += 16 * kRThreads) *(uint4 *)(d + i) = make_uint4(vv, vv, vv, vv);
    const uint32_t tail = cnt - head - body;
    if (t < tail) d[body + t] = (uint8_t)v;
}

// One workgroup per record.  A record that comes back leaves at once.  Of the others: from = the
// first difference, len = the rest of the block, and whether those len bytes of the original are all
// the value of the first of them.  Whole pieces through ld16_bounded within the block, the suffix's last
// piece, cut short, byte by byte: nothing outside the block is read.
// The workgroup votes every kRRound bytes and stops at the first piece that differs.
__global__ __launch_bounds__(kRThreads) void k_rplan(const uint32_t *__restrict__ pairs, const uint8_t *__restrict__ orig,
                                                     uint64_t n, uint32_t B, fcx_repair_entry *__restrict__ plan) {
    const uint32_t k = blockIdx.x, fd = pairs[2 * k + 1];
    if (fd == FCX_VERIFY_SAME) return;   // (the whole workgroup)
    const uint32_t blen = block_len(k, n, B);
    const uint32_t from = min(fd, blen), len = blen - from;   // (fd <= min(decoded, blen): k_vsummary)
    const uint8_t *blk = orig + (uint64_t)k * B, *p = blk + from;   // read only when len > 0
    const uint32_t v = len ? p[0] : 0u, vv = v * 0x01010101u;
    const uint32_t sp = (uint32_t)((uintptr_t)p & 15);
    bool raw = false;
    for (uint32_t base = 0; base < len; base += kRRound) {
        bool bad = false;
#pragma unroll 4
        for (uint32_t s = 0; s < kRRound / (16 * kRThreads); s++) {
            const uint32_t j = base + 16 * (s * kRThreads + threadIdx.x);
            if (j >= len) continue;
            if (j + 16 <= len) {
                const uint4 x = ld16_bounded(blk, from + j, sp, blen);
                bad |= ((x.x ^ vv) | (x.y ^ vv) | (x.z ^ vv) | (x.w ^ vv)) != 0;
            } else {
                for (uint32_t i = 0; i < len - j; i++) bad |= p[j + i] != v;
            }
        }
        if (__syncthreads_or(bad)) {   // (uniform)
            raw = true;
            break;
        }
    }
    if (threadIdx.x == 0) {
        fcx_repair_entry e;
        e.block = k;
        e.data_off = 0;
        e.from = from;
        e.len = len;
        e.kind = raw ? FCX_REPAIR_RAW : FCX_REPAIR_FILL;
        e.fill = raw ? 0u : v;
        plan[k] = e;
    }
}

// One workgroup over the records, 1024 at a time in block order: the planned entries compacted to
// entries[0, nentries) (entries may be null: the counts alone), data_off = the exclusive sum of the
// RAW lengths before the entry, the counts to the status words (zeroed before).
__global__ __launch_bounds__(1024) void k_rscan(uint32_t nblocks, const uint32_t *__restrict__ pairs,
                                                const fcx_repair_entry *__restrict__ plan,
                                                fcx_repair_entry *__restrict__ entries, uint64_t *__restrict__ words) {
    __shared__ uint32_t sh_c[16];
    __shared__ uint64_t sh_b[16];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint64_t ecarry = 0, bcarry = 0, fills = 0;
    for (uint64_t k0 = 0; k0 < nblocks; k0 += 1024) {
        const uint64_t k = k0 + t;
        const bool has = k < nblocks && pairs[2 * k + 1] != FCX_VERIFY_SAME;
        fcx_repair_entry e = {};
        if (has) e = plan[k];
        const uint64_t raw = has && e.kind == FCX_REPAIR_RAW ? e.len : 0u;
        uint32_t ci = has ? 1u : 0u;
        uint64_t bi = raw;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t c = __shfl_up(ci, o, 64);
            const uint32_t lo = __shfl_up((uint32_t)bi, o, 64), hi = __shfl_up((uint32_t)(bi >> 32), o, 64);
            if (lane >= (uint32_t)o) {
                ci += c;
                bi += ((uint64_t)hi << 32) | lo;
            }
        }
        if (lane == 63) {
            sh_c[wv] = ci;
            sh_b[wv] = bi;
        }
        __syncthreads();
        uint32_t cpre = 0, ctot = 0;
        uint64_t bpre = 0, btot = 0;
        for (uint32_t w = 0; w < 16; w++) {
            if (w < wv) {
                cpre += sh_c[w];
                bpre += sh_b[w];
            }
            ctot += sh_c[w];
            btot += sh_b[w];
        }
        __syncthreads();
        if (has) {
            if (entries) {
                e.data_off = e.kind == FCX_REPAIR_RAW ? bcarry + bpre + bi - raw : 0u;
                entries[ecarry + cpre + ci - 1] = e;
            }
            if (e.kind == FCX_REPAIR_FILL) fills++;
        }
        ecarry += ctot;
        bcarry += btot;
    }
    fills = wave_sum_u64(fills);
    if (lane == 0 && fills) atomicAdd((unsigned long long *)words + kRpFills, (unsigned long long)fills);
    if (t == 0) {
        words[kRpEntries] = ecarry;
        words[kRpData] = bcarry;
    }
}

// Workgroup (chunk c of entry e): bytes [c kRChunk, (c + 1) kRChunk) of a RAW entry's suffix of the
// original to data + data_off.  The suffix bounds the reads, [data_off, data_off + len) the writes.
__global__ __launch_bounds__(kRThreads) void k_rgather(const fcx_repair_entry *__restrict__ entries, uint32_t cpb,
                                                       const uint8_t *__restrict__ orig, uint32_t B,
                                                       uint8_t *__restrict__ data) {
    const fcx_repair_entry e = entries[blockIdx.x / cpb];
    const uint32_t lo = (blockIdx.x % cpb) * kRChunk;
    if (e.kind != FCX_REPAIR_RAW || lo >= e.len) return;   // (the whole workgroup)
    const uint8_t *src = orig + e.block * B + e.from;
    copy_aligned(data + e.data_off + lo, src + lo, min(kRChunk, e.len - lo), src, src + e.len);
}

// One thread per entry: the checks of fcx.h against the index; the first entry that fails one by
// atomicMin into kRpBadEntry, entry_of[block] for the others (preset to kNoEntry).
__global__ __launch_bounds__(kRThreads) void k_rmap(const fcx_repair_entry *__restrict__ entries, uint32_t nentries,
                                                    uint32_t nblocks, const uint64_t *__restrict__ dec_off, uint64_t n,
                                                    uint32_t B, uint64_t data_bytes, uint32_t *__restrict__ entry_of,
                                                    uint64_t *__restrict__ words) {
    const uint32_t i = blockIdx.x * kRThreads + threadIdx.x;
    if (i >= nentries) return;
    const fcx_repair_entry e = entries[i];
    bool ok = e.block < nblocks && e.kind <= FCX_REPAIR_FILL && (i == 0 || entries[i - 1].block < e.block);
    if (ok) {
        const uint64_t dlen = dec_off[e.block + 1] - dec_off[e.block];
        ok = e.from <= dlen && (uint64_t)e.from + e.len == block_len(e.block, n, B);
        if (ok && e.kind == FCX_REPAIR_RAW) ok = e.data_off <= data_bytes && e.len <= data_bytes - e.data_off;
    }
    if (!ok) {
        atomicMin((unsigned long long *)words + kRpBadEntry, (unsigned long long)i);
        return;
    }
    entry_of[e.block] = i;
    if (e.kind == FCX_REPAIR_FILL) atomicAdd((unsigned long long *)words + kRpFills, 1ull);
}

// One thread per record: without an entry it must decode to its block's length.
__global__ __launch_bounds__(kRThreads) void k_rcheck(uint32_t nblocks, const uint64_t *__restrict__ dec_off, uint64_t n,
                                                      uint32_t B, const uint32_t *__restrict__ entry_of,
                                                      uint64_t *__restrict__ words) {
    const uint32_t k = blockIdx.x * kRThreads + threadIdx.x;
    if (k >= nblocks || entry_of[k] != kNoEntry) return;
    if (dec_off[k + 1] - dec_off[k] != block_len(k, n, B))
        atomicMin((unsigned long long *)words + kRpBadRecord, (unsigned long long)k);
}

// Records [k0, k0 + nrec) of the run, decoded back to back at dec (gbytes bytes; byte 0 is decoded
// offset dec_base of the run), to their blocks of out.  Workgroup (chunk c of record r): bytes
// [c kRChunk, (c + 1) kRChunk) of block k: below the entry's `from` the decoded record's, from there on
// the entry's RAW bytes or its fill byte; a record without an entry is all decoded bytes.  The entries
// passed k_rmap, and still nothing they say moves a read out of dec[0, gbytes) or data[0, data_bytes),
// or a write out of the block: `from` is cut to the decoded and the block's length, and a RAW range
// that does not fit the data or the block is not copied.
__global__ __launch_bounds__(kRThreads) void k_rapply(const uint8_t *__restrict__ dec, uint64_t dec_base, uint64_t gbytes,
                                                      const uint64_t *__restrict__ dec_off, uint32_t k0, uint32_t cpb,
                                                      const uint32_t *__restrict__ entry_of,
                                                      const fcx_repair_entry *__restrict__ entries,
                                                      const uint8_t *__restrict__ data, uint64_t data_bytes, uint64_t n,
                                                      uint32_t B, uint8_t *__restrict__ out) {
    const uint32_t k = k0 + blockIdx.x / cpb, lo = (blockIdx.x % cpb) * kRChunk;
    const uint32_t blen = block_len(k, n, B);
    if (lo >= blen) return;   // (the whole workgroup)
    const uint32_t hi = min(blen, lo + kRChunk);
    const uint64_t d0 = dec_off[k] - dec_base;
    const uint32_t dlen = (uint32_t)min(dec_off[k + 1] - dec_off[k], gbytes - min(gbytes, d0));
    const uint32_t ei = entry_of[k];
    fcx_repair_entry e = {};
    if (ei != kNoEntry) e = entries[ei];
    const uint32_t from = ei == kNoEntry ? min(blen, dlen) : min(e.from, min(blen, dlen));
    uint8_t *dst = out + (uint64_t)k * B;
    if (lo < from) copy_aligned(dst + lo, dec + d0 + lo, min(hi, from) - lo, dec, dec + gbytes);
    if (ei == kNoEntry || hi <= from || from != e.from || (uint64_t)e.from + e.len != blen) return;
    const uint32_t a = max(lo, from);
    if (e.kind == FCX_REPAIR_FILL) {
        fill_aligned(dst + a, hi - a, e.fill);
    } else if (e.data_off <= data_bytes && e.len <= data_bytes - e.data_off) {
        copy_aligned(dst + a, data + e.data_off + (a - from), hi - a, data, data + data_bytes);
    }
}

namespace {
const char *kRBuildStages[] = {"index", "decode", "compare", "summary", "plan", "gather"};
const char *kRApplyStages[] = {"index", "check", "decode", "assemble"};

int ready_words(RepairScratch &P) {
    if (!P.host_words) {
        FCX_TRY(P.words.reserve(8 * kRpWords, "repair words"));
        FCX_HIP(P.host_words.alloc(8 * kRpWords));
    }
    return FCX_OK;
}
int ready(fcx_dctx *c) {
    for (uint64_t &v : c->rp.stats) v = 0;
    return ready_words(c->rp);
}
}  // namespace

int launch_entry_map(fcx_dctx *c, const fcx_repair_entry *d_entries, uint32_t nentries, uint32_t nblocks, uint64_t n, uint32_t B,
                     uint64_t data_bytes, bool with_check, hipStream_t st) {
    RepairScratch &P = c->rp;
    FCX_TRY(ready_words(P));
    FCX_TRY(P.entry_of.reserve(4ull * nblocks, "repair map"));
    FCX_HIP(hipMemsetAsync(P.words, 0, 8 * kRpWords, st));
    FCX_HIP(hipMemsetAsync(P.words + kRpBadEntry, 0xFF, 16, st));
    FCX_HIP(hipMemsetAsync(P.entry_of, 0xFF, 4ull * nblocks, st));
    if (nentries)
        hipLaunchKernelGGL(k_rmap, dim3((nentries + kRThreads - 1) / kRThreads), dim3(kRThreads), 0, st, d_entries, nentries,
                           nblocks, c->rg.dec_off, n, B, data_bytes, P.entry_of, P.words);
    if (with_check)
        hipLaunchKernelGGL(k_rcheck, dim3((nblocks + kRThreads - 1) / kRThreads), dim3(kRThreads), 0, st, nblocks, c->rg.dec_off, n,
                           B, P.entry_of, P.words);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(P.host_words, P.words, 8 * kRpWords, hipMemcpyDeviceToHost, st));
    return FCX_OK;
}

int entry_map_result(fcx_dctx *c, uint64_t rec_base) {
    const uint64_t *w = c->rp.host_words;
    if (w[kRpBadEntry] != ~0ull)
        return fail(FCX_ERR_FORMAT, "repair: entry " + std::to_string(w[kRpBadEntry]) + " of the records from " +
                                        std::to_string(rec_base) + " does not fit its record");
    if (w[kRpBadRecord] != ~0ull)
        return fail(FCX_ERR_FORMAT, "repair: record " + std::to_string(rec_base + w[kRpBadRecord]) +
                                        " does not decode to its block's length and has no entry");
    return FCX_OK;
}

int repair_build_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *d_orig,
                     uint64_t n, uint32_t B, fcx_repair_entry *d_entries, uint8_t *d_data, uint64_t data_cap,
                     uint32_t *nentries, uint64_t *data_bytes, uint64_t *stats, hipStream_t st, uint64_t rec_base) {
    *nentries = 0;
    *data_bytes = 0;
    uint64_t vs[FCX_VERIFY_STATS] = {0, 0, ~0ull, 0, 0, 0};
    if (stats) std::copy(vs, vs + FCX_VERIFY_STATS, stats);
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    if (nblocks == 0) return FCX_OK;
    RepairScratch &P = c->rp;
    FCX_TRY(P.pairs.reserve(8ull * nblocks, "repair pairs"));
    FCX_TRY(verify_run(c, kind, d_rec, rec_len, nblocks, d_orig, n, B, P.pairs, vs, st, rec_base));
    if (stats) std::copy(vs, vs + FCX_VERIFY_STATS, stats);
    if (vs[kVwDiffer] == 0) {   // every block comes back: no entry, and with profiling verify_run's table plus two empty stages
        if (c->profiling) c->times.publish(kRBuildStages, 6);
        return FCX_OK;
    }
    const bool prof = c->profiling;
    std::unique_ptr<StageTimes> T(prof ? new StageTimes(2) : nullptr);
    FCX_TRY(P.plan.reserve(32ull * nblocks, "repair plan"));
    FCX_HIP(hipMemsetAsync(P.words, 0, 8 * kRpWords, st));
    if (prof) T->mark(0, st);
    hipLaunchKernelGGL(k_rplan, dim3(nblocks), dim3(kRThreads), 0, st, P.pairs, d_orig, n, B, P.plan);
    hipLaunchKernelGGL(k_rscan, dim3(1), dim3(1024), 0, st, nblocks, P.pairs, P.plan, d_entries, P.words);
    if (prof) T->mark(1, st);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(P.host_words, P.words, 8 * kRpWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    const uint64_t ne = P.host_words[kRpEntries], nd = P.host_words[kRpData];
    *nentries = (uint32_t)ne;
    *data_bytes = nd;
    P.stats[0] = ne;
    P.stats[1] = P.host_words[kRpFills];
    P.stats[2] = nd;
    int rc = FCX_OK;
    if (d_entries && data_cap < nd) {
        rc = fail(FCX_ERR_CAPACITY, "fcx_repair_build_shard: data_cap is smaller than the repair's data");
    } else if (d_entries && nd) {
        const uint32_t cpb = (B + kRChunk - 1) / kRChunk;
        if (ne * cpb > kRMaxGrid) return fail(FCX_ERR_ARG, "fcx_repair_build_shard: too many entries for one call");
        hipLaunchKernelGGL(k_rgather, dim3((uint32_t)(ne * cpb)), dim3(kRThreads), 0, st, d_entries, cpb, d_orig, B, d_data);
        FCX_HIP(hipGetLastError());
    }
    if (prof) {
        T->mark(2, st);
        FCX_TRY(T->add(0, 2));
        c->times.ms[4] = T->ms[0];
        c->times.ms[5] = T->ms[1];
        c->times.publish(kRBuildStages, 6);
    } else {
        FCX_HIP(hipStreamSynchronize(st));
    }
    return rc;
}

int repair_apply_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint64_t n, uint32_t B,
                     const fcx_repair_entry *d_entries, uint32_t nentries, const uint8_t *d_data, uint64_t data_bytes,
                     uint8_t *d_out, uint64_t cap, uint64_t *out_len, hipStream_t st, uint64_t rec_base) {
    *out_len = 0;
    FCX_HIP(hipSetDevice(c->device));
    FCX_TRY(ready(c));
    if (nblocks == 0) return FCX_OK;
    RepairScratch &P = c->rp;
    VerifyScratch &V = c->vf;
    RangeScratch &R = c->rg;
    RunTimes T(c, 4, st);
    RunIndex ix;
    FCX_TRY(run_index(c, kind, d_rec, rec_len, nblocks, st, T, &ix));
    const std::vector<uint64_t> &doff = ix.doff;
    if (n == kRepairLastFromRun) {   // the last block's length from the run: its entry's, or its decoded bytes
        fcx_repair_entry last = {};
        if (nentries) FCX_HIP(hipMemcpyAsync(&last, d_entries + (nentries - 1), sizeof(last), hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        const uint64_t tail = nentries && last.block == nblocks - 1 ? (uint64_t)last.from + last.len
                                                                    : doff[nblocks] - doff[nblocks - 1];
        if (tail == 0 || tail > B)
            return fail(FCX_ERR_FORMAT, "repair: record " + std::to_string(rec_base + nblocks - 1) +
                                            " gives its block no length in [1, block size]");
        n = (uint64_t)(nblocks - 1) * B + tail;
    }
    *out_len = n;
    if (cap < n) return fail(FCX_ERR_CAPACITY, "fcx_repair_apply_shard: output capacity too small");
    FCX_TRY(launch_entry_map(c, d_entries, nentries, nblocks, n, B, data_bytes, true, st));
    T.mark(2);
    std::vector<uint32_t> eof_(nentries ? nblocks : 0);
    if (nentries) FCX_HIP(hipMemcpyAsync(eof_.data(), P.entry_of, 4ull * nblocks, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    FCX_TRY(entry_map_result(c, rec_base));
    P.stats[0] = nentries;
    P.stats[1] = P.host_words[kRpFills];
    P.stats[2] = data_bytes;
    FCX_TRY(T.add(0, 2));
    const char *who = "fcx_repair_apply_shard";
    if (nentries == 0) {   // every record decodes to its block: one full decode straight into d_out
        T.mark(2);
        FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, 0, nblocks, d_out, n, st, rec_base, who));
        T.mark(3);
        FCX_TRY(T.add(2, 3));
        P.stats[3] = 1;
    } else {
        auto staged = [&](uint32_t g0, uint32_t g1) {
            for (uint32_t k = g0; k < g1; k++)
                if (eof_[k] != kNoEntry) return true;
            return false;
        };
        std::vector<RunGroup> groups;
        FCX_TRY(run_groups(c, ix, nblocks, &groups, staged));
        const uint32_t cpb = (B + kRChunk - 1) / kRChunk;
        for (const RunGroup &g : groups) {
            const uint32_t nrec = g.g1 - g.g0;
            T.mark(2);
            if (!staged(g.g0, g.g1)) {   // (each of its records decodes to its block's length: back to back is in place)
                FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, nrec, d_out + (uint64_t)g.g0 * B, g.gbytes, st,
                                     rec_base, who));
                T.mark(3);
                T.mark(4);
                P.stats[3]++;
            } else {
                if ((uint64_t)nrec * cpb > kRMaxGrid) return fail(FCX_ERR_ARG, "fcx_repair_apply_shard: group too large");
                FCX_TRY(decode_group(c, kind, d_rec, rec_len, ix.roff, g.g0, nrec, V.buf, g.gbytes, st, rec_base, who));
                T.mark(3);
                hipLaunchKernelGGL(k_rapply, dim3(nrec * cpb), dim3(kRThreads), 0, st, V.buf, doff[g.g0], g.gbytes, R.dec_off, g.g0,
                                   cpb, P.entry_of, d_entries, d_data, data_bytes, n, B, d_out);
                T.mark(4);
                FCX_HIP(hipGetLastError());
                P.stats[4]++;
            }
            FCX_TRY(T.add(2, 4));
        }
    }
    FCX_HIP(hipStreamSynchronize(st));
    T.publish(c, kRApplyStages, 4);
    return FCX_OK;
}

}  // namespace fcx

using namespace fcx;

extern "C" {

int fcx_repair_build_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks,
                           const uint8_t *d_orig, uint64_t n, uint32_t block_bytes, fcx_repair_entry *d_entries, uint8_t *d_data,
                           uint64_t data_cap, uint32_t *nentries, uint64_t *data_bytes, uint64_t *stats, void *stream) {
    if (!nentries || !data_bytes) return fail(FCX_ERR_ARG, "fcx_repair_build_shard: NULL argument");
    FCX_TRY(run_args("fcx_repair_build_shard", c, kind, d_rec, nblocks, n, block_bytes));
    if (nblocks && !d_orig) return fail(FCX_ERR_ARG, "fcx_repair_build_shard: NULL argument");
    if ((!d_entries && d_data) || (!d_data && data_cap))
        return fail(FCX_ERR_ARG, "fcx_repair_build_shard: d_data without d_entries, or a capacity without d_data");
    return repair_build_run(c, kind, d_rec, rec_len, nblocks, d_orig, n, block_bytes, d_entries, d_data, data_cap, nentries,
                            data_bytes, stats, (hipStream_t)stream, 0);
}

int fcx_repair_apply_shard(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint64_t n,
                           uint32_t block_bytes, const fcx_repair_entry *d_entries, uint32_t nentries, const uint8_t *d_data,
                           uint64_t data_bytes, uint8_t *d_out, uint64_t cap, uint64_t *out_len, void *stream) {
    if (!out_len) return fail(FCX_ERR_ARG, "fcx_repair_apply_shard: NULL argument");
    FCX_TRY(run_args("fcx_repair_apply_shard", c, kind, d_rec, nblocks, n, block_bytes));
    if ((nentries && !d_entries) || (data_bytes && !d_data) || (n && cap && !d_out))
        return fail(FCX_ERR_ARG, "fcx_repair_apply_shard: NULL argument");
    if (cap < n) {
        *out_len = n;
        return fail(FCX_ERR_CAPACITY, "fcx_repair_apply_shard: output capacity too small");
    }
    return repair_apply_run(c, kind, d_rec, rec_len, nblocks, n, block_bytes, d_entries, nentries, d_data, data_bytes, d_out,
                            cap, out_len, (hipStream_t)stream, 0);
}

int fcx_dctx_repair_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_repair_stats: bad argument");
    for (int i = 0; i < n && i < FCX_REPAIR_STATS; i++) out[i] = c->rp.stats[i];
    return FCX_OK;
}

}  // extern "C"
