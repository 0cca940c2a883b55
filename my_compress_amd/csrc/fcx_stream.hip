// fcx_stream.hip — pipelined host I/O around the device paths.
//
// The reference's main() (my_compress.cpp:4073-4136 compress, 4137-4204
// decompress) reads a block, codes it and writes it, strictly in turn.  Here a
// file streams through two pipeline slots, each a pinned host buffer and its
// device twin: while the GPU compresses shard k, the host reads shard k+1 into
// the other slot's pinned buffer and writes shard k-1's records, and the copies
// run on their own streams (H2D, D2H) so PCIe overlaps compute as well.  Files
// larger than host memory or HBM stream through in shard-sized pieces.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"   // lz78_decompress_shard_at, the *_run forms and run_args
#include "fcx_device.h"       // the compress status words a slot's hlen mirrors
#include "fcx_host.h"
#include "fcx_digest_file.h"
#include "fcx_repair_file.h"

using namespace fcx;

namespace {

struct Slot {
    PinnedBuf<uint8_t> hin, hout;
    DevBuf<uint8_t> din, dout;
    PinnedBuf<uint64_t> hlen;   // pinned copy of the device length / error words ([kCwTotal, kCwErr])
    uint64_t n = 0;             // input bytes in this slot
    Event h2d, comp, d2h;
};

struct Pipeline {
    Slot s[2];
    Stream sin, scomp, sout;
    int device = -1;
    uint64_t in_bytes = 0, out_bytes = 0;
    int init(int dev, uint64_t in_b, uint64_t out_b) {
        device = dev;
        in_bytes = in_b;
        out_bytes = out_b;
        FCX_HIP(sin.create(hipStreamNonBlocking));
        FCX_HIP(scomp.create(hipStreamNonBlocking));
        FCX_HIP(sout.create(hipStreamNonBlocking));
        for (auto &x : s) {
            FCX_HIP(x.hin.alloc(in_bytes));
            FCX_HIP(x.hout.alloc(out_bytes));
            FCX_HIP(x.hlen.alloc(kCwHeadBytes));
            FCX_HIP(x.din.alloc(in_bytes));
            FCX_HIP(x.dout.alloc(out_bytes));
            FCX_HIP(x.h2d.create(hipEventDisableTiming));
            FCX_HIP(x.comp.create(hipEventDisableTiming));
            FCX_HIP(x.d2h.create(hipEventDisableTiming));
            FCX_HIP(hipEventRecord(x.comp, scomp));   // slots start free
            FCX_HIP(hipEventRecord(x.d2h, sout));
            FCX_HIP(hipEventRecord(x.h2d, sin));
        }
        return FCX_OK;
    }
};

// pinned/device slots are kept per host thread (one set for each direction) and
// reused while they are large enough: per-block calls do not re-pin memory
thread_local std::unique_ptr<Pipeline> g_pipe[2];

int get_pipe(int which, int dev, uint64_t in_b, uint64_t out_b, Pipeline **out) {
    std::unique_ptr<Pipeline> &p = g_pipe[which];
    if (p && (p->device != dev || p->in_bytes < in_b || p->out_bytes < out_b)) {
        (void)hipDeviceSynchronize();
        p.reset();
    }
    if (!p) {
        p.reset(new Pipeline());
        const int r = p->init(dev, in_b, out_b);
        if (r) { p.reset(); return r; }
    }
    for (auto &x : p->s) x.n = 0;
    *out = p.get();
    return FCX_OK;
}

// fills buf with up to cap bytes (short only at end of input); <0 on error
int64_t read_full(fcx_read_fn rd, void *user, uint8_t *buf, uint64_t cap) {
    uint64_t got = 0;
    while (got < cap) {
        const int64_t r = rd(user, buf + got, cap - got);
        if (r < 0) return r;
        if (r == 0) break;
        got += (uint64_t)r;
    }
    return (int64_t)got;
}

// host-to-host copies of the memory paths (a shard into / out of the pinned staging): one thread moves
// ~10 GB/s, so a 256 MiB shard's copy in and out took longer than its H2D, compress and D2H together;
// large copies are split over up to kCopyThreads threads (64-B aligned pieces of >= 8 MiB)
constexpr uint64_t kCopyPiece = 8ull << 20;
constexpr unsigned kCopyThreads = 8;
void par_memcpy(uint8_t *dst, const uint8_t *src, uint64_t n) {
    const uint64_t t = n / kCopyPiece < kCopyThreads ? n / kCopyPiece : kCopyThreads;
    if (t <= 1) { memcpy(dst, src, n); return; }
    const uint64_t per = (n / t + 63) & ~63ull;
    std::vector<std::thread> th;
    th.reserve(t - 1);
    for (uint64_t i = 1; i < t; i++) {
        const uint64_t a = i * per, b = i + 1 == t ? n : (i + 1) * per;
        if (a < b) th.emplace_back([=] { memcpy(dst + a, src + a, b - a); });
    }
    memcpy(dst, src, per < n ? per : n);
    for (auto &x : th) x.join();
}

struct MemIO {   // fcx_compress_host / fcx_decompress_* over memory
    const uint8_t *in;
    uint64_t in_len, in_pos;
    uint8_t *out;
    uint64_t cap, out_pos;
};
int64_t mem_read(void *u, uint8_t *buf, uint64_t cap) {
    MemIO *m = (MemIO *)u;
    const uint64_t n = m->in_len - m->in_pos < cap ? m->in_len - m->in_pos : cap;
    par_memcpy(buf, m->in + m->in_pos, n);
    m->in_pos += n;
    return (int64_t)n;
}
int mem_write(void *u, const uint8_t *buf, uint64_t n) {
    MemIO *m = (MemIO *)u;
    if (n > m->cap - m->out_pos) return FCX_ERR_CAPACITY;
    par_memcpy(m->out + m->out_pos, buf, n);
    m->out_pos += n;
    return 0;
}

}  // namespace

extern "C" {

int fcx_compress_stream(fcx_ctx *ctx, fcx_read_fn rd, fcx_write_fn wr, void *user, uint64_t shard_bytes,
                        uint64_t *total_in, uint64_t *total_out, uint64_t *nblocks) {
    if (!ctx || !rd || !wr) return fail(FCX_ERR_ARG, "fcx_compress_stream: NULL argument");
    uint32_t B = 0;
    int dev = 0;
    if (fcx_ctx_info(ctx, &dev, &B, nullptr)) return FCX_ERR_ARG;
    FCX_HIP(hipSetDevice(dev));
    const uint64_t shard = shard_bytes >= B ? shard_bytes / B * B : B;
    const uint64_t cap = fcx_shard_bound(shard, B);
    Pipeline *PP = nullptr;
    int r = get_pipe(0, dev, shard, cap, &PP);
    if (r) return r;
    Pipeline &P = *PP;
    const uint64_t *dlen = fcx_ctx_device_out_len(ctx);
    uint64_t tin = 0, tout = 0, tblocks = 0;
    // finish shard in slot x in two halves: length back and the records' D2H issued (start), then,
    // after the host has read the next shard into the slot's input buffer meanwhile, the D2H
    // waited for and the records written (finish)
    uint64_t olen_pending = 0;
    auto drain_start = [&](Slot &x) -> int {
        FCX_HIP(hipEventSynchronize(x.comp));
        const uint32_t e = (uint32_t)x.hlen[kCwErr];
        if (e & kErrCapacity) return fail(FCX_ERR_CAPACITY, "shard output capacity");
        if (e) return fail(FCX_ERR_INTERNAL, "device invariant violated (error bits " + std::to_string(e) + ")");
        olen_pending = x.hlen[kCwTotal];
        FCX_HIP(hipMemcpyAsync(x.hout, x.dout, olen_pending, hipMemcpyDeviceToHost, P.sout));
        FCX_HIP(hipEventRecord(x.d2h, P.sout));
        return FCX_OK;
    };
    auto drain_finish = [&](Slot &x) -> int {
        FCX_HIP(hipEventSynchronize(x.d2h));
        const int w = wr(user, x.hout, olen_pending);
        if (w) return fail(w < 0 ? w : FCX_ERR_ARG, "write callback failed");
        tout += olen_pending;
        x.n = 0;
        return FCX_OK;
    };
    auto drain = [&](Slot &x) -> int {
        const int rr = drain_start(x);
        return rr ? rr : drain_finish(x);
    };
    int64_t got = read_full(rd, user, P.s[0].hin, shard);
    if (got < 0) return fail(FCX_ERR_ARG, "read callback failed");
    for (uint32_t k = 0; got > 0; k++) {
        Slot &x = P.s[k & 1], &y = P.s[(k + 1) & 1];
        x.n = (uint64_t)got;
        tin += x.n;
        tblocks += (x.n + B - 1) / B;
        FCX_HIP(hipStreamWaitEvent(P.sin, x.comp, 0));     // x.din free again (shard k-2 compressed)
        FCX_HIP(hipMemcpyAsync(x.din, x.hin, x.n, hipMemcpyHostToDevice, P.sin));
        FCX_HIP(hipEventRecord(x.h2d, P.sin));
        FCX_HIP(hipStreamWaitEvent(P.scomp, x.h2d, 0));
        FCX_HIP(hipStreamWaitEvent(P.scomp, x.d2h, 0));   // x.dout free again
        if ((r = fcx_compress_shard(ctx, x.din, x.n, x.dout, cap, nullptr, P.scomp))) return r;
        FCX_HIP(hipMemcpyAsync(x.hlen, dlen, kCwHeadBytes, hipMemcpyDeviceToHost, P.scomp));
        FCX_HIP(hipEventRecord(x.comp, P.scomp));
        // while the GPU works on slot x: read the next shard into y (its H2D is long done)
        // and write y's finished records
        const bool last = x.n < shard;
        got = 0;
        const bool ydrain = y.n != 0;
        if (ydrain) { if ((r = drain_start(y))) return r; }
        if (!last) {   // (y.hin: its H2D is long done; y's records go out through y.hout meanwhile)
            FCX_HIP(hipEventSynchronize(y.h2d));
            got = read_full(rd, user, y.hin, shard);
            if (got < 0) return fail(FCX_ERR_ARG, "read callback failed");
        }
        if (ydrain) { if ((r = drain_finish(y))) return r; }
    }
    for (auto &x : P.s)
        if (x.n) { if ((r = drain(x))) return r; }
    if (total_in) *total_in = tin;
    if (total_out) *total_out = tout;
    if (nblocks) *nblocks = tblocks;
    return FCX_OK;
}

int fcx_compress_host(fcx_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len) {
    if (!ctx || (!in && n) || !out) return fail(FCX_ERR_ARG, "fcx_compress_host: NULL argument");
    uint64_t shard = 0;
    if (fcx_ctx_info(ctx, nullptr, nullptr, &shard)) return FCX_ERR_ARG;
    MemIO m{in, n, 0, out, cap, 0};
    const int r = fcx_compress_stream(ctx, mem_read, mem_write, &m, shard, nullptr, nullptr, nullptr);
    if (r) return r;
    if (out_len) *out_len = m.out_pos;
    return FCX_OK;
}

}  // extern "C"

namespace {

constexpr int kStopReading = 1;   // a group function's "the caller has what it wants"

// The reading half of the decompress stream paths: the header, then groups of whole records staged
// in slot 0 of the pipeline and copied to the device.  group(lz78, slot, bytes, records, out_cap,
// records before, stream) decodes one; it returns FCX_OK, an error, or kStopReading.
template <typename Group>
int stream_groups(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint32_t *hdr_total, uint64_t *nblocks,
                  Group group) {
    uint8_t hdr[FCX_HEADER_BYTES];
    if (read_full(rd, user, hdr, sizeof(hdr)) != (int64_t)sizeof(hdr)) return fail(FCX_ERR_FORMAT, "short header");
    uint32_t total = 0;
    uint16_t counted = 0;
    char kind = 0;
    int r = fcx_parse_header(hdr, &total, &counted, &kind);
    if (r) return r;
    const bool lz78 = kind != '7';   // as main() (4140-4159): anything but '7' selects LZ78
    int dev = 0;
    if (fcx_dctx_device(dctx, &dev)) return FCX_ERR_ARG;
    FCX_HIP(hipSetDevice(dev));
    // groups of whole records: up to kGroup blocks (<= 1 MiB decoded each, + 8 for FCX8) per device
    // call (max_in, when known, bounds the staging: small inputs do not pin a whole group).  An FCX7
    // record is <= 2 len + 4096 bytes and a group's staging holds kGroup of them; an FCX8 record may
    // be 10 len + 4096, so its groups close at kGroup records or when the next record no longer fits
    // the staging of kIn78 bytes (>= 12 records of the largest size).
    constexpr uint32_t kGroup = 256;
    constexpr uint64_t kIn78 = 128ull << 20;
    const uint64_t len_max = lz78 ? 10ull * FCX_MAX_BLOCK_BYTES + 4096 : 2ull * FCX_MAX_BLOCK_BYTES + 4096;
    const uint64_t blk_max = lz78 ? FCX_MAX_BLOCK_BYTES + 8ull : FCX_MAX_BLOCK_BYTES;
    uint64_t in_cap = lz78 ? kIn78 : (uint64_t)kGroup * (len_max + 4);
    uint64_t out_cap = (uint64_t)kGroup * blk_max;
    if (max_in && max_in < in_cap) {
        in_cap = max_in;
        // each record of >= 4 + 3 bytes decodes to <= 1 MiB (+ 8)
        out_cap = blk_max * ((max_in + 6) / 7 < kGroup ? (max_in + 6) / 7 : kGroup);
    }
    Pipeline *PP = nullptr;
    if ((r = get_pipe(1, dev, in_cap, out_cap, &PP))) return r;
    Pipeline &P = *PP;
    Slot &x = P.s[0];
    uint64_t tblocks = 0;
    // FCX8: the header's counted records and no more (main() reads block_num records, 4162-4201)
    uint64_t left = lz78 ? counted : ~0ull;
    bool eof = false, have_len = false;
    uint32_t len = 0;   // (have_len: the length of a record that did not fit the group before)
    while (!eof && left) {
        uint64_t used = 0;
        uint32_t nb = 0;
        while (nb < kGroup && left) {
            if (!have_len) {
                const int64_t g = read_full(rd, user, (uint8_t *)&len, 4);
                if (g == 0 && !lz78) { eof = true; break; }
                if (g != 4) return fail(FCX_ERR_FORMAT, "truncated block record");
                if (len > len_max) return fail(FCX_ERR_FORMAT, "block record too long");
            }
            have_len = false;
            if (used + 4 + (uint64_t)len > in_cap) {
                if (!lz78 || nb == 0) return fail(FCX_ERR_FORMAT, "truncated block record");
                have_len = true;   // opens the next group
                break;
            }
            memcpy(x.hin + used, &len, 4);
            if (read_full(rd, user, x.hin + used + 4, len) != (int64_t)len)
                return fail(FCX_ERR_FORMAT, "truncated block record");
            used += 4 + (uint64_t)len;
            nb++;
            left--;
        }
        if (nb == 0) break;
        FCX_HIP(hipMemcpyAsync(x.din, x.hin, used, hipMemcpyHostToDevice, P.scomp));
        r = group(lz78, x, used, nb, out_cap, tblocks, P.scomp);
        tblocks += nb;
        if (r == kStopReading) break;
        if (r) return r;
    }
    if (hdr_total) *hdr_total = total;
    if (nblocks) *nblocks = tblocks;
    return FCX_OK;
}

// ---- what the group functions of the stream forms share ----

// a group's got decoded bytes at x.dout to the write callback
int write_group(Slot &x, uint64_t got, fcx_write_fn wr, void *user, hipStream_t st, uint64_t *tout) {
    FCX_HIP(hipMemcpyAsync(x.hout, x.dout, got, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    const int w = wr(user, x.hout, got);
    if (w) return fail(w < 0 ? w : FCX_ERR_ARG, "write callback failed");
    *tout += got;
    return FCX_OK;
}

// a stream form's checks of run_args: it has no run in hand yet
int block_arg(const char *fn, fcx_dctx *c, uint32_t block_bytes) { return run_args(fn, c, '7', nullptr, 0, 0, block_bytes); }

// The group's nb blocks of the original to x.dout, staged where a decompress stages the decoded bytes (every
// record is >= 7 bytes of a staging that holds 1 MiB of output per 7 bytes of input); *got: their bytes.
int stage_original(const char *fn, fcx_read_fn rd_orig, void *user_orig, Slot &x, uint32_t nb, uint64_t B, uint64_t out_cap,
                   bool *orig_end, uint64_t *got, hipStream_t st) {
    const uint64_t want = (uint64_t)nb * B;
    if (want > out_cap) return fail(FCX_ERR_INTERNAL, std::string(fn) + ": staging too small");
    const int64_t g = *orig_end ? 0 : read_full(rd_orig, user_orig, x.hout, want);
    if (g < 0) return fail(FCX_ERR_ARG, "read callback failed");
    if ((uint64_t)g < want) *orig_end = true;
    if (g) FCX_HIP(hipMemcpyAsync(x.dout, x.hout, (uint64_t)g, hipMemcpyHostToDevice, st));
    *got = (uint64_t)g;
    return FCX_OK;
}

// The entries of records [before, before + nb) (F null: none), their sections read now and no further:
// block and data_off rebased to the group, to rp.entries, their RAW bytes to rp.data.
int load_entries(fcx_dctx *dctx, fcx_repair_file::Reader *F, uint64_t before, uint32_t nb, std::vector<fcx_repair_entry> *ents,
                 std::vector<uint8_t> *raw, hipStream_t st) {
    ents->clear();
    raw->clear();
    while (F) {
        fcx_repair_entry e;
        const uint8_t *bytes = nullptr;
        const int g = F->next(before, before + nb, &e, &bytes);
        if (g < 0) return fail(g, F->err);
        if (g == 0) break;
        e.block -= before;
        e.data_off = 0;
        if (e.kind == FCX_REPAIR_RAW) {
            e.data_off = raw->size();
            raw->insert(raw->end(), bytes, bytes + e.len);
        }
        ents->push_back(e);
    }
    RepairScratch &P = dctx->rp;
    FCX_TRY(P.entries.reserve(sizeof(fcx_repair_entry) * ents->size(), "repair entries"));
    FCX_TRY(P.data.reserve(raw->size(), "repair data"));
    if (!ents->empty())
        FCX_HIP(hipMemcpyAsync(P.entries, ents->data(), sizeof(fcx_repair_entry) * ents->size(), hipMemcpyHostToDevice, st));
    if (!raw->empty()) FCX_HIP(hipMemcpyAsync(P.data, raw->data(), raw->size(), hipMemcpyHostToDevice, st));
    return FCX_OK;
}

// a group's six stats into the running sum of the file's, the first failing block numbered file-wide
void fold_stats(uint64_t *sum, const uint64_t *gs, uint64_t before) {
    if (gs[2] != ~0ull && sum[2] == ~0ull) sum[2] = before + gs[2];
    for (int i : {0, 1, 3, 4, 5}) sum[i] += gs[i];
}

// the end of a verify or check stream: bytes of the original behind the last record count as differing
// and are reported last, with block = the number of records
int finish_stats(uint64_t *sum, uint64_t extra, fcx_verify_fn on_block, void *user_cb, uint64_t *stats) {
    sum[4] += extra;
    if (extra && on_block) on_block(user_cb, sum[0], extra, 0, 0);
    for (int i = 0; i < FCX_VERIFY_STATS; i++) stats[i] = sum[i];
    return FCX_OK;
}

// passes a read callback through and keeps the first bytes that went by: the FCX file's header, for the
// kind of a file without records (stream_groups calls no group then)
struct PeekRead {
    fcx_read_fn rd;
    void *user;
    uint8_t hdr[FCX_HEADER_BYTES];
    uint64_t seen;
};
int64_t peek_read(void *u, uint8_t *buf, uint64_t cap) {
    PeekRead *p = (PeekRead *)u;
    const int64_t r = p->rd(p->user, buf, cap);
    for (int64_t i = 0; i < r && p->seen < sizeof(p->hdr); i++) p->hdr[p->seen++] = buf[i];
    return r;
}

// the repair file's codec against a group's `kind`; kind 0, behind the last group: a file without records
// has its header to go by
int codec_check(const fcx_repair_file::Reader &F, char kind, const PeekRead &pk, uint64_t records) {
    if (!kind && records == 0 && pk.seen == sizeof(pk.hdr)) kind = pk.hdr[3] == '7' ? '7' : '8';
    if (kind && kind != F.kind) return fail(FCX_ERR_FORMAT, "repair file: made for the other codec");
    return FCX_OK;
}

constexpr uint64_t kDgShard = 64ull << 20;   // bytes of the original per device call of fcx_digest_stream

}  // namespace

extern "C" {

int fcx_decompress_stream(fcx_dctx *dctx, fcx_read_fn rd, fcx_write_fn wr, void *user, uint64_t max_in,
                          uint32_t *hdr_total, uint64_t *total_out, uint64_t *nblocks) {
    if (!dctx || !rd || !wr) return fail(FCX_ERR_ARG, "fcx_decompress_stream: NULL argument");
    uint64_t tout = 0;
    const int r = stream_groups(dctx, rd, user, max_in, hdr_total, nblocks,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t before,
                                    hipStream_t st) -> int {
        uint64_t got = 0;
        if (lz78) FCX_TRY(fcx::lz78_decompress_shard_at(dctx, x.din, used, nb, x.dout, out_cap, &got, st, before));
        else FCX_TRY(fcx_decompress_shard(dctx, x.din, used, nb, x.dout, out_cap, &got, st));
        return write_group(x, got, wr, user, st, &tout);
    });
    if (r) return r;
    if (total_out) *total_out = tout;
    return FCX_OK;
}

int fcx_decompress_range_stream(fcx_dctx *dctx, fcx_read_fn rd, fcx_write_fn wr, void *user, uint64_t max_in, uint64_t off,
                                uint64_t len, uint64_t *total_out) {
    if (!dctx || !rd || !wr) return fail(FCX_ERR_ARG, "fcx_decompress_range_stream: NULL argument");
    uint64_t pos = 0, tout = 0;   // decoded bytes before the group, bytes written
    const uint64_t end = len < ~0ull - off ? off + len : ~0ull;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t before,
                                    hipStream_t st) -> int {
        // the group's part of the range, in the group's decoded bytes (empty before the range starts:
        // the call then only indexes the group, for its decoded size)
        const uint64_t lo = off > pos ? off - pos : 0, n = end > pos + lo ? end - pos - lo : 0;
        uint64_t got = 0, gtotal = 0;
        FCX_TRY(fcx::range_shard(dctx, lz78 ? '8' : '7', x.din, used, nb, nullptr, nullptr, lo, n, x.dout, out_cap, &got, st,
                                 before, &gtotal));
        if (got) FCX_TRY(write_group(x, got, wr, user, st, &tout));
        pos += gtotal;
        return pos >= end ? kStopReading : FCX_OK;
    });
    if (r) return r;
    if (total_out) *total_out = tout;
    return FCX_OK;
}

int fcx_decompress_range_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, uint64_t off, uint64_t len, uint8_t *out,
                              uint64_t cap, uint64_t *out_len) {
    if (!dctx || !in || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_decompress_range_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO m{in, in_len, 0, out, cap, 0};
    FCX_TRY(fcx_decompress_range_stream(dctx, mem_read, mem_write, &m, in_len - FCX_HEADER_BYTES, off, len, nullptr));
    *out_len = m.out_pos;
    return FCX_OK;
}

// Original bytes left after the last record are counted (read and dropped through the staging of
// slot 0), added to stats[4] and reported by a last on_block call with block = the number of records.
int fcx_verify_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, fcx_read_fn rd_orig, void *user_orig,
                      uint32_t block_bytes, uint64_t max_in, fcx_verify_fn on_block, void *user_cb, uint64_t *stats) {
    if (!dctx || !rd || !rd_orig || !stats) return fail(FCX_ERR_ARG, "fcx_verify_stream: NULL argument");
    FCX_TRY(block_arg("fcx_verify_stream", dctx, block_bytes));
    const uint64_t B = block_bytes;
    uint64_t sum[FCX_VERIFY_STATS] = {0, 0, ~0ull, 0, 0, 0};
    std::vector<uint32_t> pairs;
    bool orig_end = false;
    uint8_t *spare = nullptr;   // (pinned staging of slot 0, for the bytes after the last record)
    uint64_t spare_cap = 0;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t before,
                                    hipStream_t st) -> int {
        spare = x.hout;
        spare_cap = out_cap;
        uint64_t got = 0;
        FCX_TRY(stage_original("fcx_verify_stream", rd_orig, user_orig, x, nb, B, out_cap, &orig_end, &got, st));
        FCX_TRY(dctx->vf.blocks.reserve(8ull * nb, "verify pairs"));
        uint64_t gs[FCX_VERIFY_STATS];
        FCX_TRY(fcx::verify_run(dctx, lz78 ? '8' : '7', x.din, used, nb, x.dout, got, block_bytes, dctx->vf.blocks, gs, st,
                                before));
        pairs.resize(2ull * nb);
        FCX_HIP(hipMemcpy(pairs.data(), dctx->vf.blocks, 8ull * nb, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < nb && on_block; k++) {
            if (pairs[2 * k + 1] == FCX_VERIFY_SAME) continue;
            const uint64_t o0 = (uint64_t)k * B, blen = o0 < got ? std::min(B, got - o0) : 0;
            on_block(user_cb, before + k, blen, pairs[2 * k], pairs[2 * k + 1]);
        }
        fold_stats(sum, gs, before);
        return FCX_OK;
    });
    if (r) return r;
    uint64_t extra = 0;
    if (!orig_end) {
        uint8_t small[4096];
        uint8_t *buf = spare ? spare : small;
        const uint64_t cap = spare ? spare_cap : sizeof(small);
        for (;;) {
            const int64_t got = rd_orig(user_orig, buf, cap);
            if (got < 0) return fail(FCX_ERR_ARG, "read callback failed");
            if (got == 0) break;
            extra += (uint64_t)got;
        }
    }
    return finish_stats(sum, extra, on_block, user_cb, stats);
}

int fcx_verify_host(fcx_dctx *dctx, char kind, const uint8_t *rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *orig,
                    uint64_t n, uint32_t block_bytes, uint32_t *blocks_host, uint64_t *stats) {
    if (!dctx || !stats || (rec_len && !rec) || (n && !orig)) return fail(FCX_ERR_ARG, "fcx_verify_host: NULL argument");
    int dev = 0;
    if (fcx_dctx_device(dctx, &dev)) return FCX_ERR_ARG;
    FCX_HIP(hipSetDevice(dev));
    DevBuf<uint8_t> d_rec, d_orig;
    DevBuf<uint32_t> d_blocks;
    FCX_TRY(d_rec.reserve(rec_len, "records"));
    FCX_TRY(d_orig.reserve(n, "original"));
    if (blocks_host) FCX_TRY(d_blocks.reserve(8ull * nblocks, "verify pairs"));
    if (rec_len) FCX_HIP(hipMemcpy(d_rec, rec, rec_len, hipMemcpyHostToDevice));
    if (n) FCX_HIP(hipMemcpy(d_orig, orig, n, hipMemcpyHostToDevice));
    FCX_TRY(fcx_verify_shard(dctx, kind, d_rec, rec_len, nblocks, d_orig, n, block_bytes, blocks_host ? d_blocks.p : nullptr,
                             stats, nullptr));
    if (blocks_host && nblocks) FCX_HIP(hipMemcpy(blocks_host, d_blocks, 8ull * nblocks, hipMemcpyDeviceToHost));
    return FCX_OK;
}

int fcx_decompress_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap,
                        uint64_t *out_len) {
    if (!dctx || !in || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_decompress_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO m{in, in_len, 0, out, cap, 0};
    const int r = fcx_decompress_stream(dctx, mem_read, mem_write, &m, in_len - FCX_HEADER_BYTES, nullptr, nullptr,
                                        nullptr);
    if (r) return r;
    if (out_len) *out_len = m.out_pos;
    return FCX_OK;
}

// ---- the repair sidecar's stream and host forms (include/fcx.h) ----------------------

int fcx_repair_build_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, fcx_read_fn rd_orig, void *user_orig,
                            uint32_t block_bytes, uint64_t max_in, fcx_write_fn wr, void *user_wr, uint64_t *stats) {
    if (!dctx || !rd || !rd_orig || !wr) return fail(FCX_ERR_ARG, "fcx_repair_build_stream: NULL argument");
    FCX_TRY(block_arg("fcx_repair_build_stream", dctx, block_bytes));
    const uint64_t B = block_bytes;
    fcx_repair_file::Writer W(wr, user_wr);
    PeekRead pk{rd, user, {}, 0};
    bool begun = false, orig_end = false;
    uint64_t total_n = 0, records = 0;
    std::vector<fcx_repair_entry> ents;
    std::vector<uint8_t> raw;
    const int r = stream_groups(dctx, peek_read, &pk, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t before,
                                    hipStream_t st) -> int {
        if (!begun) {
            if (const int w = W.begin(lz78 ? '8' : '7', block_bytes)) return fail(w, W.err);
            begun = true;
        }
        uint64_t got = 0;
        FCX_TRY(stage_original("fcx_repair_build_stream", rd_orig, user_orig, x, nb, B, out_cap, &orig_end, &got, st));
        if ((got + B - 1) / B != nb)
            return fail(FCX_ERR_ARG, "fcx_repair_build_stream: the original has no bytes for record " +
                                         std::to_string(before + (got + B - 1) / B));
        RepairScratch &P = dctx->rp;
        FCX_TRY(P.entries.reserve(sizeof(fcx_repair_entry) * (uint64_t)nb, "repair entries"));
        FCX_TRY(P.data.reserve(got, "repair data"));   // (the RAW bytes are bytes of the group's blocks)
        uint32_t ne = 0;
        uint64_t nd = 0;
        FCX_TRY(fcx::repair_build_run(dctx, lz78 ? '8' : '7', x.din, used, nb, x.dout, got, block_bytes, P.entries, P.data, got,
                                      &ne, &nd, nullptr, st, before));
        ents.resize(ne);
        raw.resize(nd);
        if (ne) FCX_HIP(hipMemcpy(ents.data(), P.entries, sizeof(fcx_repair_entry) * (uint64_t)ne, hipMemcpyDeviceToHost));
        if (nd) FCX_HIP(hipMemcpy(raw.data(), P.data, nd, hipMemcpyDeviceToHost));
        for (fcx_repair_entry e : ents) {
            const uint8_t *bytes = e.kind == FCX_REPAIR_RAW ? raw.data() + e.data_off : nullptr;
            e.block += before;
            if (const int w = W.add(e, bytes)) return fail(w, W.err);
        }
        total_n += got;
        records += nb;
        return FCX_OK;
    });
    if (r) return r;
    if (!orig_end) {
        uint8_t one;
        const int64_t got = rd_orig(user_orig, &one, 1);
        if (got < 0) return fail(FCX_ERR_ARG, "read callback failed");
        if (got) return fail(FCX_ERR_ARG, "fcx_repair_build_stream: the original has bytes after the last record");
    }
    if (!begun)
        if (const int w = W.begin(pk.hdr[3] == '7' ? '7' : '8', block_bytes)) return fail(w, W.err);
    if (const int w = W.finish(total_n, records)) return fail(w, W.err);
    if (stats) {
        stats[0] = total_n;
        stats[1] = records;
        stats[2] = W.entries;
        stats[3] = W.data_bytes;
    }
    return FCX_OK;
}

int fcx_repair_apply_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, fcx_read_fn rd_rep, void *user_rep, fcx_write_fn wr,
                            void *user_out, uint64_t max_in, uint64_t *total_out) {
    if (!dctx || !rd || !rd_rep || !wr) return fail(FCX_ERR_ARG, "fcx_repair_apply_stream: NULL argument");
    fcx_repair_file::Reader F(rd_rep, user_rep);
    if (const int f = F.open()) return fail(f, F.err);
    const uint32_t B = F.block_bytes;
    PeekRead pk{rd, user, {}, 0};
    uint64_t tout = 0, records = 0;
    bool short_seen = false;
    std::vector<fcx_repair_entry> ents;
    std::vector<uint8_t> raw;
    const int r = stream_groups(dctx, peek_read, &pk, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t before,
                                    hipStream_t st) -> int {
        FCX_TRY(codec_check(F, lz78 ? '8' : '7', pk, records));
        if (short_seen)
            return fail(FCX_ERR_FORMAT, "repair: record " + std::to_string(before - 1) +
                                            " gives a block shorter than the block size and is not the last");
        if ((uint64_t)nb * B > out_cap) return fail(FCX_ERR_INTERNAL, "fcx_repair_apply_stream: staging too small");
        FCX_TRY(load_entries(dctx, &F, before, nb, &ents, &raw, st));
        RepairScratch &P = dctx->rp;
        uint64_t n = 0;
        FCX_TRY(fcx::repair_apply_run(dctx, lz78 ? '8' : '7', x.din, used, nb, fcx::kRepairLastFromRun, B, P.entries,
                                      (uint32_t)ents.size(), P.data, raw.size(), x.dout, out_cap, &n, st, before));
        if (n < (uint64_t)nb * B) short_seen = true;
        records += nb;
        return write_group(x, n, wr, user_out, st, &tout);
    });
    if (r) return r;
    FCX_TRY(codec_check(F, 0, pk, records));
    if (const int f = F.finish(tout, records)) return fail(f, F.err);
    if (total_out) *total_out = tout;
    return FCX_OK;
}

int fcx_repair_build_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, const uint8_t *orig, uint64_t n,
                          uint32_t block_bytes, uint8_t *repair, uint64_t cap, uint64_t *repair_len) {
    if (!dctx || !in || (n && !orig) || !repair_len || (cap && !repair))
        return fail(FCX_ERR_ARG, "fcx_repair_build_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO comp{in, in_len, 0, nullptr, 0, 0}, org{orig, n, 0, nullptr, 0, 0}, out{nullptr, 0, 0, repair, cap, 0};
    const int r = fcx_repair_build_stream(dctx, mem_read, &comp, mem_read, &org, block_bytes, in_len - FCX_HEADER_BYTES, mem_write,
                                          &out, nullptr);
    *repair_len = out.out_pos;
    return r == FCX_ERR_CAPACITY ? fail(r, "fcx_repair_build_host: repair capacity too small") : r;
}

int fcx_repair_apply_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, const uint8_t *repair, uint64_t repair_len,
                          uint8_t *out, uint64_t cap, uint64_t *out_len) {
    if (!dctx || !in || !repair || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_repair_apply_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO comp{in, in_len, 0, nullptr, 0, 0}, rep{repair, repair_len, 0, nullptr, 0, 0}, dst{nullptr, 0, 0, out, cap, 0};
    const int r = fcx_repair_apply_stream(dctx, mem_read, &comp, mem_read, &rep, mem_write, &dst, in_len - FCX_HEADER_BYTES,
                                          nullptr);
    *out_len = dst.out_pos;
    return r == FCX_ERR_CAPACITY ? fail(r, "fcx_repair_apply_host: output capacity too small") : r;
}

// ---- the content digest's check, stream and host forms (include/fcx.h) ---------------

int fcx_check_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, fcx_read_fn rd_rep, void *user_rep, fcx_read_fn rd_dig,
                     void *user_dig, uint64_t max_in, fcx_verify_fn on_block, void *user_cb, uint64_t *stats) {
    if (!dctx || !rd || !rd_dig || !stats) return fail(FCX_ERR_ARG, "fcx_check_stream: NULL argument");
    fcx_digest_file::Reader G(rd_dig, user_dig);
    if (const int g = G.open()) return fail(g, G.err);
    const uint32_t block_bytes = G.block_bytes;
    const uint64_t B = block_bytes;
    fcx_repair_file::Reader F(rd_rep, user_rep);
    if (rd_rep) {
        if (const int f = F.open()) return fail(f, F.err);
        if (F.block_bytes != block_bytes) return fail(FCX_ERR_FORMAT, "repair file: made for another block size than the digest file's");
    }
    PeekRead pk{rd, user, {}, 0};
    uint64_t sum[FCX_VERIFY_STATS] = {0, 0, ~0ull, 0, 0, 0};
    uint64_t result_bytes = 0, records = 0;
    std::vector<uint32_t> want, pairs;
    std::vector<fcx_repair_entry> ents;
    std::vector<uint8_t> raw;
    const int r = stream_groups(dctx, peek_read, &pk, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        if (rd_rep) FCX_TRY(codec_check(F, lz78 ? '8' : '7', pk, records));
        // the group's values: the sections that hold them are read now, and no further; whether the
        // group's last block is the file's last, and so shorter, shows once the sections have ended
        want.clear();
        const int64_t got = G.take(nb, &want);
        if (got < 0) return fail((int)got, G.err);
        const int m = G.more();
        if (m < 0) return fail(m, G.err);
        uint64_t n = (uint64_t)got * B;
        if (m == 0 && got) n = (uint64_t)(got - 1) * B + G.block_len(before + (uint64_t)got - 1);
        FCX_TRY(load_entries(dctx, rd_rep ? &F : nullptr, before, nb, &ents, &raw, st));
        RepairScratch &P = dctx->rp;
        DigestScratch &D = dctx->dg;
        FCX_TRY(D.crc.reserve(4ull * nb, "digest values"));
        FCX_TRY(D.blocks.reserve(8ull * nb, "digest pairs"));
        if (got) FCX_HIP(hipMemcpyAsync(D.crc, want.data(), 4ull * (uint64_t)got, hipMemcpyHostToDevice, st));
        uint64_t gs[FCX_VERIFY_STATS];
        FCX_TRY(fcx::check_run(dctx, lz78 ? '8' : '7', x.din, used, nb, (uint32_t)got, n, block_bytes, P.entries,
                               (uint32_t)ents.size(), P.data, raw.size(), D.crc, D.blocks, gs, st, before));
        pairs.resize(2ull * nb);
        FCX_HIP(hipMemcpy(pairs.data(), D.blocks, 8ull * nb, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < nb; k++) {
            const uint64_t o0 = (uint64_t)k * B, blen = k < (uint64_t)got && o0 < n ? std::min(B, n - o0) : 0;
            result_bytes += pairs[2 * k];
            if (on_block && (k >= (uint64_t)got || pairs[2 * k] != blen || pairs[2 * k + 1] != want[k]))
                on_block(user_cb, before + k, blen, pairs[2 * k], pairs[2 * k + 1]);
        }
        fold_stats(sum, gs, before);
        records += nb;
        return FCX_OK;
    });
    if (r) return r;
    if (rd_rep) {
        FCX_TRY(codec_check(F, 0, pk, records));
        if (const int f = F.finish(result_bytes, records)) return fail(f, F.err);
    }
    // blocks of the digest file behind the last record
    const int64_t left = G.take(~0ull, nullptr);
    if (left < 0) return fail((int)left, G.err);
    if (const int g = G.finish()) return fail(g, G.err);
    return finish_stats(sum, left ? G.n - std::min(G.n, records * B) : 0, on_block, user_cb, stats);
}

int fcx_check_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, const uint8_t *repair, uint64_t repair_len,
                   const uint8_t *digest, uint64_t digest_len, fcx_verify_fn on_block, void *user_cb, uint64_t *stats) {
    if (!dctx || !in || !digest || !stats) return fail(FCX_ERR_ARG, "fcx_check_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO comp{in, in_len, 0, nullptr, 0, 0}, rep{repair, repair_len, 0, nullptr, 0, 0}, dig{digest, digest_len, 0, nullptr, 0, 0};
    return fcx_check_stream(dctx, mem_read, &comp, repair ? mem_read : nullptr, &rep, mem_read, &dig, in_len - FCX_HEADER_BYTES,
                            on_block, user_cb, stats);
}

// ---- the search's stream and host forms (include/fcx.h) ------------------------------

int fcx_find_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, const uint8_t *pattern, uint32_t plen,
                    fcx_hit_fn on_hit, void *user_cb, uint64_t *stats) {
    if (!dctx || !rd || !pattern) return fail(FCX_ERR_ARG, "fcx_find_stream: NULL argument");
    if (plen < 1 || plen > FCX_FIND_MAX_PATTERN)
        return fail(FCX_ERR_ARG, "fcx_find_stream: pattern length outside [1, FCX_FIND_MAX_PATTERN]");
    uint64_t sum[4] = {0, 0, 0, 0};
    FindSink sink;
    sink.on_hit = on_hit;
    sink.user = user_cb;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        if (before == 0) dctx->fd.carry_len = 0;   // a new search; later groups go on from the carry
        uint64_t hits = 0, dec = 0;
        FCX_TRY(fcx::find_run(dctx, lz78 ? '8' : '7', x.din, used, nb, pattern, plen, sum[1], sink, &hits, &dec, st, before));
        sum[0] += hits;
        sum[1] += dec;
        sum[2] += nb;
        sum[3] += dctx->fd.stats[0];
        return FCX_OK;
    });
    if (r) return r;
    for (int i = 0; i < 4 && stats; i++) stats[i] = sum[i];
    return FCX_OK;
}

int fcx_find_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, const uint8_t *pattern, uint32_t plen, uint64_t *hits,
                  uint64_t cap, uint64_t *nhits) {
    if (!dctx || !in || !pattern || !nhits || (cap && !hits)) return fail(FCX_ERR_ARG, "fcx_find_host: NULL argument");
    if (plen < 1 || plen > FCX_FIND_MAX_PATTERN)
        return fail(FCX_ERR_ARG, "fcx_find_host: pattern length outside [1, FCX_FIND_MAX_PATTERN]");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    struct Take {
        uint64_t *hits, cap, n;
    } take{hits, cap, 0};
    MemIO comp{in, in_len, 0, nullptr, 0, 0};
    uint64_t stats[4] = {};
    const fcx_hit_fn keep = [](void *u, uint64_t off) {
        Take *k = (Take *)u;
        if (k->n < k->cap) k->hits[k->n] = off;
        k->n++;
    };
    FCX_TRY(fcx_find_stream(dctx, mem_read, &comp, in_len - FCX_HEADER_BYTES, pattern, plen, cap ? keep : nullptr, &take, stats));
    *nhits = stats[0];
    return FCX_OK;
}

}  // extern "C"

// ---- the line calls' stream and host forms (include/fcx.h) ---------------------------

namespace {

// The groups of a file as one run of lines: `each` prepares the group's request (the decoded base, the
// delimiters so far and the last delimiter are already in it), `after` sees its result and may end the reading.
// sum: delimiters, 1 + the position of the last one, decoded bytes.
template <typename Each, typename After>
int lines_groups(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, uint64_t *sum, Each each,
                        After after) {
    sum[0] = sum[1] = sum[2] = 0;
    return stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                         [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        LinesReq q;
        q.delim = delim;
        q.base = sum[2];
        q.nl_before = sum[0];
        q.last_before = sum[1];
        q.last_run = false;   // (whether a group is the file's last shows only at the end of the reading)
        each(&q, st);
        LinesRes res;
        FCX_TRY(fcx::lines_run(dctx, lz78 ? '8' : '7', x.din, used, nb, q, &res, st, before));
        sum[0] = res.nl;
        sum[1] = res.last;
        sum[2] += res.decoded;
        return after(q, res, st);
    });
}

void lines_file_stats(const uint64_t *sum, uint64_t *stats) {
    stats[0] = sum[0];
    stats[1] = sum[0] + (sum[2] > 0 && sum[1] != sum[2]);
    stats[2] = sum[2];
    stats[3] = sum[2] - std::min(sum[1], sum[2]);
}

}  // namespace

extern "C" {

int fcx_lines_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, uint64_t *stats) {
    if (!dctx || !rd || !stats) return fail(FCX_ERR_ARG, "fcx_lines_stream: NULL argument");
    uint64_t sum[3];
    FCX_TRY(lines_groups(dctx, rd, user, max_in, delim, sum, [](LinesReq *, hipStream_t) {}, [](const LinesReq &, const LinesRes &, hipStream_t) { return FCX_OK; }));
    lines_file_stats(sum, stats);
    return FCX_OK;
}

int fcx_lines_locate_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, uint64_t first,
                            uint64_t count, uint64_t *off, uint64_t *len) {
    if (!dctx || !rd || !off || !len) return fail(FCX_ERR_ARG, "fcx_lines_locate_stream: NULL argument");
    const uint64_t r[2] = {first, count < ~0ull - first ? first + count : ~0ull};
    uint64_t found[2] = {r[0] ? ~0ull : 0, r[1] ? ~0ull : 0};   // 1 + the position of each boundary delimiter; ~0: not seen yet
    uint64_t sum[3];
    FCX_TRY(lines_groups(dctx, rd, user, max_in, delim, sum,
                         [&](LinesReq *q, hipStream_t) {
                             for (int i = 0; i < 2; i++) q->sel[i] = found[i] == ~0ull ? r[i] : ~0ull;
                             q->stop_early = true;
                         },
                         [&](const LinesReq &q, const LinesRes &res, hipStream_t) {
                             for (int i = 0; i < 2; i++)
                                 if (q.sel[i] != ~0ull) found[i] = res.sel[i];
                             return found[0] != ~0ull && found[1] != ~0ull ? kStopReading : FCX_OK;
                         }));
    // a boundary the file does not hold is its end: the reading went to it, so sum[2] is T
    *off = found[0] == ~0ull ? sum[2] : found[0];
    *len = (found[1] == ~0ull ? sum[2] : found[1]) - *off;
    return FCX_OK;
}

int fcx_lines_of_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, const uint64_t *offsets,
                        uint64_t noff, uint64_t *lines) {
    if (!dctx || !rd || (noff && (!offsets || !lines))) return fail(FCX_ERR_ARG, "fcx_lines_of_stream: NULL argument");
    for (uint64_t i = 1; i < noff; i++)
        if (offsets[i - 1] > offsets[i]) return fail(FCX_ERR_ARG, "fcx_lines_of_stream: offset " + std::to_string(i) + " descends");
    uint64_t done = 0, take = 0;   // offsets answered, the group's slice
    uint64_t sum[3];
    FCX_TRY(lines_groups(dctx, rd, user, max_in, delim, sum,
                         [&](LinesReq *q, hipStream_t st) {
                             // the offsets in [base, base + decoded) go to the device once the group's size is known
                             q->staged = [&, st](uint64_t decoded, LinesReq *r) -> int {
                                 const uint64_t *lo = offsets + done, *hi = std::lower_bound(lo, offsets + noff, r->base + decoded);
                                 take = (uint64_t)(hi - lo);
                                 if (!take) return FCX_OK;
                                 LinesScratch &S = dctx->ln;
                                 FCX_TRY(S.offs.reserve(8 * take, "line offsets"));
                                 FCX_TRY(S.lines.reserve(8 * take, "line numbers"));
                                 FCX_HIP(hipMemcpyAsync(S.offs, lo, 8 * take, hipMemcpyHostToDevice, st));
                                 FCX_HIP(hipStreamSynchronize(st));
                                 r->d_offsets = S.offs;
                                 r->noff = take;
                                 r->d_lines = S.lines;
                                 return FCX_OK;
                             };
                         },
                         [&](const LinesReq &, const LinesRes &, hipStream_t st) -> int {
                             if (take) {
                                 FCX_HIP(hipMemcpyAsync(lines + done, dctx->ln.lines, 8 * take, hipMemcpyDeviceToHost, st));
                                 FCX_HIP(hipStreamSynchronize(st));
                             }
                             done += take;
                             take = 0;
                             return FCX_OK;   // (groups behind the last offset are still read: an offset may be the file's end)
                         }));
    for (; done < noff; done++) {   // what is left lies at the file's end, or behind it
        if (offsets[done] > sum[2])
            return fail(FCX_ERR_ARG, "fcx_lines_of_stream: offset " + std::to_string(done) + " lies behind the file's end");
        lines[done] = sum[0];
    }
    return FCX_OK;
}

int fcx_lines_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, uint8_t delim, uint64_t *stats) {
    if (!dctx || !in || !stats) return fail(FCX_ERR_ARG, "fcx_lines_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO comp{in, in_len, 0, nullptr, 0, 0};
    return fcx_lines_stream(dctx, mem_read, &comp, in_len - FCX_HEADER_BYTES, delim, stats);
}

int fcx_decompress_lines_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, uint8_t delim, uint64_t first, uint64_t count,
                              uint8_t *out, uint64_t cap, uint64_t *out_len) {
    if (!dctx || !in || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_decompress_lines_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO comp{in, in_len, 0, nullptr, 0, 0};
    uint64_t off = 0, len = 0;
    *out_len = 0;
    FCX_TRY(fcx_lines_locate_stream(dctx, mem_read, &comp, in_len - FCX_HEADER_BYTES, delim, first, count, &off, &len));
    *out_len = len;
    if (len > cap) return fail(FCX_ERR_CAPACITY, "fcx_decompress_lines_host: output capacity too small");
    if (len == 0) return FCX_OK;
    return fcx_decompress_range_host(dctx, in, in_len, off, len, out, len, out_len);
}

int fcx_lines_of_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, uint8_t delim, const uint64_t *offsets, uint64_t noff,
                      uint64_t *lines) {
    if (!dctx || !in || (noff && (!offsets || !lines))) return fail(FCX_ERR_ARG, "fcx_lines_of_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    MemIO comp{in, in_len, 0, nullptr, 0, 0};
    return fcx_lines_of_stream(dctx, mem_read, &comp, in_len - FCX_HEADER_BYTES, delim, offsets, noff, lines);
}

// ---- the grep's and the multi-range decode's stream forms (include/fcx.h) ------------

int fcx_grep_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, const uint8_t *pattern,
                    uint32_t plen, fcx_range_fn on_line, void *user_line, uint64_t *stats) {
    if (!dctx || !rd || !pattern) return fail(FCX_ERR_ARG, "fcx_grep_stream: NULL argument");
    if (plen < 1 || plen > FCX_FIND_MAX_PATTERN)
        return fail(FCX_ERR_ARG, "fcx_grep_stream: pattern length outside [1, FCX_FIND_MAX_PATTERN]");
    if (memchr(pattern, delim, plen)) return fail(FCX_ERR_ARG, "fcx_grep_stream: the pattern holds the delimiter");
    GrepSink sink;
    sink.on_line = on_line;
    sink.user = user_line;
    GrepCarry carry;
    uint64_t gs[FCX_GREP_STATS] = {};
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        return fcx::grep_run(dctx, lz78 ? '8' : '7', x.din, used, nb, delim, pattern, plen, sink, &carry, gs, st, before);
    });
    if (r) return r;
    if (carry.held) {   // the file ends inside a selected line
        if (on_line) on_line(user_line, carry.held_start, carry.base);
        carry.held = false;
    }
    // (the bytes of a line still open at the end: the words hold its start, with or without a callback)
    if (gs[0] && dctx->gp.host_words && dctx->gp.host_words[kGwOpen]) gs[1] += carry.base - dctx->gp.host_words[kGwLast];
    gs[4] = carry.base;
    for (int i = 0; i < FCX_GREP_STATS && stats; i++) stats[i] = gs[i];
    return FCX_OK;
}

// ---- the pattern sets' stream and host forms (include/fcx.h): where the file ends shows only when
// the reader has ended, so the positions the last group carried are judged by a final pass over the carry alone ----

int fcx_find_set_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, const fcx_pattern_set *set, fcx_hit_fn on_hit,
                        void *user_cb, uint64_t *stats, uint64_t *counts) {
    if (!dctx || !rd || !set) return fail(FCX_ERR_ARG, "fcx_find_set_stream: NULL argument");
    FCX_TRY(fcx::set_args("fcx_find_set_stream", set, -1));
    uint64_t sum[4] = {0, 0, 0, 0};
    FindSink sink;
    sink.on_hit = on_hit;
    sink.user = user_cb;
    hipStream_t last_st = nullptr;
    bool any = false;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        uint64_t hits = 0, dec = 0;
        FCX_TRY(fcx::find_set_run(dctx, lz78 ? '8' : '7', x.din, used, nb, set, sum[1], sink, false, &hits, &dec, counts, st, before));
        sum[0] += hits;
        sum[1] += dec;
        sum[2] += nb;
        last_st = st;
        any = true;
        return FCX_OK;
    });
    if (r) return r;
    if (any) {
        uint64_t hits = 0;
        FCX_TRY(fcx::find_set_final(dctx, set, sum[1], sink, &hits, counts, last_st));
        sum[0] += hits;
    } else {   // a file without records: nothing ran, so nothing of an earlier call may show
        uint64_t none = 0;
        FCX_TRY(fcx::find_set_run(dctx, '7', nullptr, 0, 0, set, 0, sink, true, &none, nullptr, counts, nullptr, 0));
    }
    sum[3] = dctx->ps.stats[0];
    for (int i = 0; i < 4 && stats; i++) stats[i] = sum[i];
    return FCX_OK;
}

int fcx_find_set_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, const fcx_pattern_set *set, uint64_t *hits, uint64_t cap,
                      uint64_t *nhits, uint64_t *counts) {
    if (!dctx || !in || !set || !nhits || (cap && !hits)) return fail(FCX_ERR_ARG, "fcx_find_set_host: NULL argument");
    FCX_TRY(fcx::set_args("fcx_find_set_host", set, -1));
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    struct Take {
        uint64_t *hits, cap, n;
    } take{hits, cap, 0};
    MemIO comp{in, in_len, 0, nullptr, 0, 0};
    uint64_t stats[4] = {};
    const fcx_hit_fn keep = [](void *u, uint64_t off) {
        Take *k = (Take *)u;
        if (k->n < k->cap) k->hits[k->n] = off;
        k->n++;
    };
    FCX_TRY(fcx_find_set_stream(dctx, mem_read, &comp, in_len - FCX_HEADER_BYTES, set, cap ? keep : nullptr, &take, stats, counts));
    *nhits = stats[0];
    return FCX_OK;
}

int fcx_grep_set_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, const fcx_pattern_set *set,
                        fcx_range_fn on_line, void *user_line, uint64_t *stats, uint64_t *counts) {
    if (!dctx || !rd || !set) return fail(FCX_ERR_ARG, "fcx_grep_set_stream: NULL argument");
    FCX_TRY(fcx::set_args("fcx_grep_set_stream", set, delim));
    GrepSink sink;
    sink.on_line = on_line;
    sink.user = user_line;
    GrepCarry carry;
    uint64_t gs[FCX_GREP_STATS] = {};
    hipStream_t last_st = nullptr;
    bool any = false;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        last_st = st;
        any = true;
        return fcx::grep_set_run(dctx, lz78 ? '8' : '7', x.din, used, nb, delim, set, sink, &carry, gs, counts, st, before);
    });
    if (r) return r;
    if (any) FCX_TRY(fcx::grep_set_final(dctx, delim, set, sink, &carry, gs, counts, last_st));
    else FCX_TRY(fcx::grep_set_run(dctx, '7', nullptr, 0, 0, delim, set, sink, &carry, gs, counts, nullptr, 0));
    if (carry.held) {   // the file ends inside a selected line
        if (on_line) on_line(user_line, carry.held_start, carry.base);
        carry.held = false;
    }
    if (gs[0] && dctx->gp.host_words && dctx->gp.host_words[kGwOpen]) gs[1] += carry.base - dctx->gp.host_words[kGwLast];
    gs[4] = carry.base;
    for (int i = 0; i < FCX_GREP_STATS && stats; i++) stats[i] = gs[i];
    return FCX_OK;
}

// ---- context and inverted grep (include/fcx.h): fcx_grep_set_stream's shape; the run's end, which
// closes the open line and the open block, shows only when the reader has ended ----
int fcx_grep_blocks_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, uint8_t delim, const fcx_pattern_set *set,
                           const fcx_grep_opts *opts, fcx_block_fn on_block, void *user_block, uint64_t *stats, uint64_t *counts) {
    if (!dctx || !rd || !set) return fail(FCX_ERR_ARG, "fcx_grep_blocks_stream: NULL argument");
    FCX_TRY(fcx::blocks_args("fcx_grep_blocks_stream", set, delim, opts));
    BlockSink sink;
    sink.on_block = on_block;
    sink.user = user_block;
    BlockCarry carry;
    uint64_t gs[FCX_GREP_BLOCK_STATS] = {};
    hipStream_t last_st = nullptr;
    bool any = false;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        last_st = st;
        any = true;
        return fcx::blocks_run(dctx, lz78 ? '8' : '7', x.din, used, nb, delim, set, *opts, sink, &carry, gs, counts, st, before);
    });
    if (r) return r;
    if (any) FCX_TRY(fcx::blocks_final(dctx, delim, set, *opts, sink, &carry, gs, counts, last_st));
    else FCX_TRY(fcx::blocks_run(dctx, '7', nullptr, 0, 0, delim, set, *opts, sink, &carry, gs, counts, nullptr, 0));
    gs[6] = carry.base;
    for (int i = 0; i < FCX_GREP_BLOCK_STATS && stats; i++) stats[i] = gs[i];
    return FCX_OK;
}

// ---- regular-expression grep (include/fcx.h): fcx_grep_blocks_stream with the regex's run functions ----
int fcx_grep_regex_blocks_stream(fcx_dctx *dctx, fcx_read_fn rd, void *user, uint64_t max_in, const fcx_regex *re,
                                 const fcx_grep_opts *opts, fcx_block_fn on_block, void *user_block, uint64_t *stats) {
    if (!dctx || !rd || !re) return fail(FCX_ERR_ARG, "fcx_grep_regex_blocks_stream: NULL argument");
    FCX_TRY(fcx::regex_args("fcx_grep_regex_blocks_stream", re, opts));
    BlockSink sink;
    sink.on_block = on_block;
    sink.user = user_block;
    BlockCarry carry;
    uint64_t gs[FCX_GREP_BLOCK_STATS] = {};
    hipStream_t last_st = nullptr;
    bool any = false;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t, uint64_t before, hipStream_t st) -> int {
        last_st = st;
        any = true;
        return fcx::regex_run(dctx, lz78 ? '8' : '7', x.din, used, nb, re, *opts, sink, &carry, gs, st, before);
    });
    if (r) return r;
    if (any) FCX_TRY(fcx::regex_final(dctx, re, *opts, sink, &carry, gs, last_st));
    else FCX_TRY(fcx::regex_run(dctx, '7', nullptr, 0, 0, re, *opts, sink, &carry, gs, nullptr, 0));
    gs[6] = carry.base;
    for (int i = 0; i < FCX_GREP_BLOCK_STATS && stats; i++) stats[i] = gs[i];
    return FCX_OK;
}

// ---- cut (include/fcx.h): fcx_decompress_stream's twin.  The file is one text: the open line's ticks and
// the counters stay in the context's words from group to group, each group's kept bytes go through `wr` ----
int fcx_cut_stream(fcx_dctx *dctx, fcx_read_fn rd, fcx_write_fn wr, void *user, uint64_t max_in, const fcx_cut *cut, uint64_t *stats) {
    if (!dctx || !rd || !cut) return fail(FCX_ERR_ARG, "fcx_cut_stream: NULL argument");
    uint64_t tout = 0, groups = 0, gs[FCX_CUT_STATS] = {};
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t before, hipStream_t st) -> int {
        uint64_t got = 0;
        // (the output is a subsequence of the group's decoded bytes, which the staging holds)
        FCX_TRY(fcx::cut_run(dctx, lz78 ? '8' : '7', x.din, used, nb, cut, wr ? (uint8_t *)x.dout : nullptr, wr ? out_cap : 0, &got, gs, st,
                             before, before != 0));
        groups += gs[5];
        if (!wr || got == 0) {
            tout += got;
            return FCX_OK;
        }
        return write_group(x, got, wr, user, st, &tout);
    });
    if (r) return r;
    gs[0] = tout;
    gs[5] = groups;
    for (int i = 0; i < FCX_CUT_STATS; i++) dctx->ct.stats[i] = gs[i];
    for (int i = 0; i < FCX_CUT_STATS && stats; i++) stats[i] = gs[i];
    return FCX_OK;
}

int fcx_cut_host(fcx_dctx *dctx, const uint8_t *in, uint64_t in_len, const fcx_cut *cut, uint8_t *out, uint64_t cap, uint64_t *out_len,
                 uint64_t *stats) {
    if (!dctx || !in || !cut || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_cut_host: NULL argument");
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0) return fail(FCX_ERR_FORMAT, "not an FCX stream");
    *out_len = 0;
    // what fits is stored, the rest counted: the total is known when the file ends
    struct Take {
        uint8_t *out;
        uint64_t cap, n;
    } take{out, cap, 0};
    struct Both {
        MemIO comp;
        Take *take;
    } io{{in, in_len, 0, nullptr, 0, 0}, &take};
    const fcx_read_fn rd = [](void *u, uint8_t *buf, uint64_t n) { return mem_read(&((Both *)u)->comp, buf, n); };
    const fcx_write_fn wr = [](void *u, const uint8_t *buf, uint64_t n) {
        Take *k = ((Both *)u)->take;
        if (k->n < k->cap) par_memcpy(k->out + k->n, buf, std::min(n, k->cap - k->n));
        k->n += n;
        return 0;
    };
    uint64_t gs[FCX_CUT_STATS] = {};
    FCX_TRY(fcx_cut_stream(dctx, rd, cap ? wr : nullptr, &io, in_len - FCX_HEADER_BYTES, cut, gs));
    for (int i = 0; i < FCX_CUT_STATS && stats; i++) stats[i] = gs[i];
    *out_len = gs[0];
    if (gs[0] > cap) return fail(FCX_ERR_CAPACITY, "fcx_cut_host: output capacity too small");
    return FCX_OK;
}

int fcx_decompress_ranges_stream(fcx_dctx *dctx, fcx_read_fn rd, fcx_write_fn wr, void *user, uint64_t max_in,
                                 const uint64_t *starts, const uint64_t *ends, uint64_t n, uint64_t *out_len) {
    if (!dctx || !rd || !wr || (n && (!starts || !ends))) return fail(FCX_ERR_ARG, "fcx_decompress_ranges_stream: NULL argument");
    for (uint64_t i = 0; i < n; i++)
        if (starts[i] > ends[i] || (i && ends[i - 1] > starts[i]))
            return fail(FCX_ERR_ARG, "fcx_decompress_ranges_stream: range " + std::to_string(i) +
                                         " breaks start <= end or starts in front of the end of the range before it");
    if (out_len) *out_len = 0;
    if (n == 0) return FCX_OK;         // nothing to decode: nothing is read
    uint64_t done = 0;                 // ranges that lie wholly in front of the groups still to come
    uint64_t pos = 0, tout = 0;        // decoded bytes before the group, bytes written
    std::vector<uint64_t> gs, ge;
    const int r = stream_groups(dctx, rd, user, max_in, nullptr, nullptr,
                                [&](bool lz78, Slot &x, uint64_t used, uint32_t nb, uint64_t out_cap, uint64_t, hipStream_t st) -> int {
        const char kind = lz78 ? '8' : '7';
        RangeScratch &R = dctx->rg;
        RangesScratch &Q = dctx->rq;
        FCX_TRY(R.rec_off.reserve(8ull * nb + 8, "index"));
        FCX_TRY(R.dec_off.reserve(8ull * nb + 8, "index"));
        uint64_t gtotal = 0;
        FCX_TRY(fcx_index_shard(dctx, kind, x.din, used, nb, R.rec_off, R.dec_off, &gtotal, st));
        const uint64_t hi = pos + gtotal;
        // the slice of the ranges that meets [pos, hi), clipped to it and counted from the group's first byte
        gs.clear();
        ge.clear();
        for (uint64_t i = done; i < n && starts[i] < hi; i++) {
            const uint64_t s = std::max(starts[i], pos), e = std::min(ends[i], hi);
            if (s < e) {
                gs.push_back(s - pos);
                ge.push_back(e - pos);
            }
        }
        while (done < n && ends[done] <= hi) done++;
        pos = hi;
        if (!gs.empty()) {
            FCX_TRY(Q.starts.reserve(8 * gs.size(), "ranges"));
            FCX_TRY(Q.ends.reserve(8 * gs.size(), "ranges"));
            FCX_HIP(hipMemcpyAsync(Q.starts, gs.data(), 8 * gs.size(), hipMemcpyHostToDevice, st));
            FCX_HIP(hipMemcpyAsync(Q.ends, ge.data(), 8 * ge.size(), hipMemcpyHostToDevice, st));
            uint64_t got = 0;
            FCX_TRY(fcx::ranges_run(dctx, kind, x.din, used, nb, R.rec_off, R.dec_off, Q.starts, Q.ends, gs.size(), x.dout, out_cap, &got, st));
            if (got) FCX_TRY(write_group(x, got, wr, user, st, &tout));
        }
        return done == n ? kStopReading : FCX_OK;
    });
    if (r) return r;
    if (out_len) *out_len = tout;
    if (done < n)
        return fail(FCX_ERR_ARG, "fcx_decompress_ranges_stream: range " + std::to_string(done) + " ends behind the file's end");
    return FCX_OK;
}

int fcx_digest_stream(fcx_dctx *c, fcx_read_fn rd, void *user, uint32_t block_bytes, fcx_write_fn wr, void *user_wr,
                      uint64_t *stats) {
    if (!c || !rd || !wr) return fail(FCX_ERR_ARG, "fcx_digest_stream: NULL argument");
    FCX_TRY(block_arg("fcx_digest_stream", c, block_bytes));
    FCX_HIP(hipSetDevice(c->device));
    const uint64_t B = block_bytes, shard = kDgShard / B * B;
    fcx_digest_file::Writer W(wr, user_wr);
    if (const int w = W.begin(block_bytes)) return fail(w, W.err);
    DigestScratch &D = c->dg;
    std::vector<uint8_t> host;
    std::vector<uint32_t> vals;
    for (bool end = false; !end;) {
        host.resize(shard);
        const int64_t r = read_full(rd, user, host.data(), shard);
        if (r < 0) return fail(FCX_ERR_ARG, "read callback failed");
        const uint64_t got = (uint64_t)r;
        end = got < shard;
        if (got == 0) break;
        const uint32_t nb = (uint32_t)((got + B - 1) / B);
        FCX_TRY(D.stage.reserve(shard, "digest staging"));
        FCX_TRY(D.crc.reserve(4ull * (shard / B), "digest values"));
        FCX_HIP(hipMemcpyAsync(D.stage, host.data(), got, hipMemcpyHostToDevice, nullptr));
        FCX_TRY(fcx::digest_run(c, D.stage, got, block_bytes, D.crc, nullptr, nullptr));
        vals.resize(nb);
        FCX_HIP(hipMemcpy(vals.data(), D.crc, 4ull * nb, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < nb; k++)
            if (const int w = W.add(vals[k], std::min<uint64_t>(B, got - k * B))) return fail(w, W.err);
    }
    if (const int w = W.finish()) return fail(w, W.err);
    if (stats) {
        stats[0] = W.n;
        stats[1] = W.blocks;
        stats[2] = W.whole;
    }
    return FCX_OK;
}

int fcx_digest_host(fcx_dctx *c, const uint8_t *orig, uint64_t n, uint32_t block_bytes, uint8_t *digest, uint64_t cap,
                    uint64_t *digest_len) {
    if (!c || (n && !orig) || !digest_len || (cap && !digest)) return fail(FCX_ERR_ARG, "fcx_digest_host: NULL argument");
    MemIO src{orig, n, 0, nullptr, 0, 0}, dst{nullptr, 0, 0, digest, cap, 0};
    const int r = fcx_digest_stream(c, mem_read, &src, block_bytes, mem_write, &dst, nullptr);
    *digest_len = dst.out_pos;
    return r == FCX_ERR_CAPACITY ? fail(r, "fcx_digest_host: digest capacity too small") : r;
}

}  // extern "C"
