// fcx_dec_shared.h — device code and context shared by the GPU decoders: fcx_dec.hip (FCX7) and
// fcx_lz78_dec.hip (FCX8).  The sequential bit reader, the Huffman table probes, the segment
// decoder (Jacobi-synchronised parallel entropy decode) and the block scan live here once.
#ifndef FCX_DEC_SHARED_H
#define FCX_DEC_SHARED_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <vector>

#include "fcx_host.h"

namespace fcx {

// device error bits of the decoders
constexpr uint32_t kDErrRecord = 1, kDErrHeader = 2, kDErrTree = 4, kDErrGolomb = 8, kDErrDist = 16,
                   kDErrOutCap = 32, kDErrScratch = 64,
                   kDErrIndex = 128;   // a range decode: a touched record's size is not the index's

// the FCX7 sub-streams a pass gives room in the symbol scratch and decodes, bit q = sub-stream q (flags,
// chars, distances, Golomb bytes): no decoded size depends on the chars or the distances, so the size
// pass leaves them out
constexpr uint32_t kAllStreams = 0xFu, kSizeStreams = 0x9u;

// window of a range decode in the decoded bytes of the records being expanded: byte lo goes to d_out[0]
struct DClip {
    uint64_t lo = 0, hi = 0;
};

constexpr uint32_t kDSymThreads = 1024;
constexpr uint32_t kDTblBits = 10;

struct DStream {         // one Huffman sub-stream (or the raw flags byte)
    uint64_t words_bit;  // absolute bit offset of the code words in the input
    uint64_t pairs_off;  // byte offset of the (l, r) pairs; bitmap is just before
    uint64_t dst;        // byte offset of the decoded symbols in the symbol scratch
    uint32_t nbits;      // 32 W
    uint32_t count;      // symbols to produce
    uint32_t ts;         // internal nodes (0: single symbol, decodes as zeros)
    uint32_t raw;        // 1: no Huffman stream, `rawv` is the one flags byte (nb <= 1)
    uint32_t rawv;
    uint32_t pad;
};

__device__ inline uint32_t ld_u32le(const uint8_t *p, uint64_t off) {
    return p[off] | (p[off + 1] << 8) | (p[off + 2] << 16) | ((uint32_t)p[off + 3] << 24);
}

// ---------------------------------------------------------------------------
// LSB-first sequential bit reader: a 64-bit register buffer fed from a queue of
// four dwords (one 16-B load), with the next 16-B load in flight: the wait for a
// load falls every 128 bits consumed, one load behind.  The byte buffer of `len`
// bytes starts at bit `bit0` of its 16-B-aligned base.
struct BitBuf {
    const uint32_t *w;   // 16-B-aligned base
    uint64_t nw;         // dwords that hold valid bytes
    uint64_t buf, ni;    // ni: next 16-B unit to load
    uint32_t nbuf, qn, q0, q1, q2, q3;
    uint4 nxt;
    __device__ uint4 load4(uint64_t i) const {
        if (4 * i + 4 <= nw) return ((const uint4 *)w)[i];
        uint4 v;
        v.x = 4 * i < nw ? w[4 * i] : 0u;
        v.y = 4 * i + 1 < nw ? w[4 * i + 1] : 0u;
        v.z = 4 * i + 2 < nw ? w[4 * i + 2] : 0u;
        v.w = 4 * i + 3 < nw ? w[4 * i + 3] : 0u;
        return v;
    }
    __device__ uint32_t pop() {
        const uint32_t v = q0;
        q0 = q1; q1 = q2; q2 = q3;
        if (--qn == 0) {
            q0 = nxt.x; q1 = nxt.y; q2 = nxt.z; q3 = nxt.w;
            qn = 4;
            nxt = load4(ni++);
        }
        return v;
    }
    __device__ void refill() {
        if (nbuf <= 32) { buf |= (uint64_t)pop() << nbuf; nbuf += 32; }
    }
    __device__ void seek(uint64_t absbit) {   // afterwards >= 33 bits are buffered
        const uint64_t wi = absbit >> 5, i4 = wi >> 2;
        const uint4 c = load4(i4);
        nxt = load4(i4 + 1);
        ni = i4 + 2;
        const uint32_t skip = (uint32_t)(wi & 3);
        q0 = c.x; q1 = c.y; q2 = c.z; q3 = c.w;
        qn = 4;
        for (uint32_t k = 0; k < skip; k++) (void)pop();
        buf = pop();
        nbuf = 32;
        buf >>= (absbit & 31);
        nbuf -= (uint32_t)(absbit & 31);
        refill();
    }
    __device__ uint32_t peek() const { return (uint32_t)buf; }
    __device__ void drop(uint32_t n) { buf >>= n; nbuf -= n; refill(); }   // n <= 32
};

__device__ inline BitBuf make_bits(const uint8_t *buf, uint64_t len, uint64_t &bit0) {
    const uintptr_t a = (uintptr_t)buf;
    BitBuf s;
    s.w = (const uint32_t *)(a & ~(uintptr_t)15);
    bit0 = 8 * (a & 15);
    s.nw = ((a & 15) + len + 3) / 4;
    s.buf = 0; s.ni = 0; s.nbuf = 0; s.qn = 0; s.q0 = s.q1 = s.q2 = s.q3 = 0;
    s.nxt = make_uint4(0, 0, 0, 0);
    return s;
}

// one Huffman symbol from the low bits of a 32-bit window; len = 0 if none
__device__ inline uint32_t huff_sym(uint32_t win, const uint16_t *T, const uint16_t *C, uint32_t &len) {
    const uint32_t e = T[win & ((1u << kDTblBits) - 1)];
    if (!(e & 0x8000u)) { len = (e >> 8) & 0x1Fu; return e & 0xFFu; }
    len = 0;
    if (e == 0xFFFFu) return 0;
    uint32_t node = e & 0x1FFu;
    win >>= kDTblBits;
    for (uint32_t d = kDTblBits + 1; d <= 32; d++) {   // codes are <= 32 bits (k_dtable)
        const uint32_t nx = C[2 * node + (win & 1u)];
        win >>= 1;
        if (nx < 256) { len = d; return nx; }
        node = nx - 256;
    }
    return 0;
}

// The wide form of the same probe, for alphabets past 256 symbols (the FCX8 group ids, up to
// ~4100): T is 1024 u32 entries (handed over as u16 *), bit 31 clear: symbol | len << 16; bit 31
// set: continue from internal node (entry & 0x7FFF) after 10 bits; 0xFFFFFFFF invalid.  C holds
// 2 u16 children per node: bit 15 set = internal node (low 15 bits), else the leaf's symbol.
constexpr uint32_t kWideNode = 0x8000u;
__device__ inline uint32_t huff_sym_wide(uint32_t win, const uint16_t *T, const uint16_t *C, uint32_t &len) {
    const uint32_t e = ((const uint32_t *)T)[win & ((1u << kDTblBits) - 1)];
    if (!(e & 0x80000000u)) { len = (e >> 16) & 0x3Fu; return e & 0xFFFFu; }
    len = 0;
    if (e == 0xFFFFFFFFu) return 0;
    uint32_t node = e & 0x7FFFu;
    win >>= kDTblBits;
    for (uint32_t d = kDTblBits + 1; d <= 32; d++) {   // codes are <= 32 bits (the table builder checks)
        const uint32_t nx = C[2 * node + (win & 1u)];
        win >>= 1;
        if (!(nx & kWideNode)) { len = d; return nx; }
        node = nx & 0x7FFFu;
    }
    return 0;
}

// the code kinds the segment decoder walks
constexpr int kCodeHuff = 0, kCodeGolomb = 1, kCodeHuffWide = 2;

// one code at relative bit `pos` (the reader is positioned there); false if the
// stream cannot supply it.  Golomb-Rice (golomb_rice_decode 309-358): q ones, a
// zero, r in 2 bits, value 4q + r.
template <int MODE>
__device__ inline bool code_step(BitBuf &bb, uint32_t &pos, uint32_t nbits, const uint16_t *T, const uint16_t *C,
                                 uint32_t &v) {
    if (MODE != kCodeGolomb) {
        uint32_t len;
        v = MODE == kCodeHuffWide ? huff_sym_wide(bb.peek(), T, C, len) : huff_sym(bb.peek(), T, C, len);
        if (len == 0 || pos + len > nbits) return false;
        bb.drop(len);
        pos += len;
        return true;
    }
    uint32_t q = 0;
    for (;;) {
        const uint32_t w = bb.peek();
        if (w == 0xFFFFFFFFu) {
            q += 32;
            pos += 32;
            if (pos + 3 > nbits) return false;
            bb.drop(32);
            continue;
        }
        const uint32_t ones = (uint32_t)__builtin_ctz(~w);
        q += ones;
        pos += ones;
        if (pos + 3 > nbits) return false;
        bb.drop(ones);
        v = 4 * q + ((bb.peek() >> 1) & 3u);
        bb.drop(3);
        pos += 3;
        return true;
    }
}

// Segment decoder: one workgroup decodes `count` symbols of an nbits stream at
// absolute bit sb.  Lane i owns bits [i S, (i+1) S) (S = nbits / lanes, a multiple
// of 32) and decodes the codes that START there.  The first code boundary in each
// segment is agreed by a Jacobi fixed point, start_{i+1} = exit of segment i
// walked from start_i; only lanes whose start moved walk again.  Huffman codes
// resynchronise within a few symbols, so this settles in 2-3 rounds; past
// kDMaxRounds the lanes walk one after another (exact, serial).  Then a scan of
// the counts and a second walk that stores the symbols: bytes at dst8 (kCodeHuff), u32 at
// dst32 (kCodeGolomb), u16 at (uint16_t *)dst32 (kCodeHuffWide).  Returns symbols produced.
constexpr uint32_t kDMaxRounds = 12;
constexpr uint32_t kDMinSegBits = 256;
constexpr uint32_t kDRetryScale = 16;   // an unsettled stream retries with segments this much longer
// its statistics block, u64 each (where a decoder keeps the block: its status-word table)
constexpr uint32_t kSsRounds = 0, kSsFallbacks = 1;   // Jacobi rounds, serial fallbacks
constexpr uint32_t kSsGolomb = 2;                     // the same pair for the golomb walk (k_dgolomb's stats)
constexpr uint32_t kSsKind = 4;                       // Huffman fallbacks per sub-stream kind: flags, chars, p, golomb
constexpr uint32_t kSsWords = 8;

template <int MODE>
__device__ uint32_t seg_decode(const BitBuf &src, uint64_t sb, uint32_t nbits, uint32_t count, const uint16_t *T,
                               const uint16_t *C, uint8_t *dst8, uint32_t *dst32, uint32_t *st, uint32_t *cnt,
                               uint32_t *flag, uint64_t *stats) {
    constexpr bool GOLOMB = MODE == kCodeGolomb;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr uint32_t kW = kDSymThreads / 64;
    // segments of >= kDMinSegBits (Jacobi needs room to resynchronise), a multiple of 32
    const uint32_t S0 = max(kDMinSegBits, ((nbits + kDSymThreads - 1) / kDSymThreads + 31) & ~31u);
    uint32_t seg_lo = 0, seg_hi = 0;
    auto walk = [&](uint32_t start, uint32_t &ex) -> uint32_t {
        BitBuf bb = src;
        uint32_t pos = start, n = 0, v;
        bool ok = true;
        if (pos < seg_hi) bb.seek(sb + pos);
        while (pos < seg_hi) {
            if (!code_step<MODE>(bb, pos, nbits, T, C, v)) { ok = false; break; }
            n++;
        }
        ex = ok ? pos : nbits;   // a code that cannot complete ends the stream
        return n;
    };
    bool settled = false;
    uint32_t rounds = 0, mine = 0, ex = 0, n = 0;
    // codes that resynchronise slowly (near fixed-length, e.g. the packed distance
    // bytes) may not settle within short segments: a second attempt uses longer ones
    for (uint32_t attempt = 0; attempt < 2 && !settled; attempt++) {
        const uint64_t S = attempt == 0 ? S0 : (uint64_t)S0 * kDRetryScale;
        seg_lo = (uint32_t)min<uint64_t>(tid * S, nbits);
        seg_hi = (uint32_t)min<uint64_t>(seg_lo + S, nbits);
        __syncthreads();
        st[tid] = seg_lo;
        if (tid == 0) { flag[0] = 0; flag[1] = 0; }
        __syncthreads();
        mine = seg_lo;
        n = walk(mine, ex);
        for (uint32_t round = 0; round < kDMaxRounds; round++) {
            if (tid == 0) flag[(round + 1) & 1] = 0;
            if (tid + 1 < kDSymThreads && st[tid + 1] != ex) { st[tid + 1] = ex; flag[round & 1] = 1; }
            __syncthreads();
            rounds++;
            if (!flag[round & 1]) { settled = true; break; }
            if (st[tid] != mine) { mine = st[tid]; n = walk(mine, ex); }
            __syncthreads();
        }
    }
    if (!settled) {   // serial fallback over the long segments: every start exact before its lane walks
        const uint32_t active = (uint32_t)min<uint64_t>(kDSymThreads, (nbits + (uint64_t)S0 * kDRetryScale - 1) /
                                                                         ((uint64_t)S0 * kDRetryScale));
        for (uint32_t i = 0; i < active; i++) {
            if (tid == i) {
                mine = st[i];
                n = walk(mine, ex);
                if (i + 1 < kDSymThreads) st[i + 1] = ex;
            }
            __syncthreads();
        }
        mine = st[tid];
        if (tid >= active) n = 0;
    }
    if (tid == 0 && stats) {   // Jacobi rounds, serial fallbacks
        atomicAdd((unsigned long long *)stats + kSsRounds, (unsigned long long)rounds);
        if (!settled) atomicAdd((unsigned long long *)stats + kSsFallbacks, 1ull);
        if (!settled && MODE == kCodeHuff) atomicAdd((unsigned long long *)stats + kSsKind + (blockIdx.x & 3), 1ull);
    }
    // exclusive scan of the per-lane counts
    uint32_t inc = n;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += t;
    }
    if (lane == 63) cnt[wv] = inc;
    __syncthreads();
    uint32_t idx = inc - n, tot = 0;
    for (uint32_t w = 0; w < kW; w++) {
        if (w < wv) idx += cnt[w];
        tot += cnt[w];
    }
    // walk again and store
    if (mine < seg_hi && idx < count) {
        BitBuf bb = src;
        uint32_t pos = mine, v;
        bb.seek(sb + pos);
        const uint32_t stop = min(count, idx + n);
        if (GOLOMB) {
            while (idx < stop && code_step<MODE>(bb, pos, nbits, T, C, v)) dst32[idx++] = v;
        } else if (MODE == kCodeHuffWide) {
            uint16_t *dst16 = (uint16_t *)dst32;
            while (idx < stop && code_step<MODE>(bb, pos, nbits, T, C, v)) dst16[idx++] = (uint16_t)v;
        } else {
            // whole dwords inside this lane's range are stored at once; the partial
            // dwords at its two ends (shared with neighbours) byte by byte
            const uint32_t first = idx;
            uint32_t acc = 0;
            while (idx < stop && code_step<MODE>(bb, pos, nbits, T, C, v)) {
                acc |= v << (8 * (idx & 3));
                if ((idx & 3) == 3) {
                    if (idx - 3 >= first) ((uint32_t *)dst8)[idx >> 2] = acc;
                    else
                        for (uint32_t q = first; q <= idx; q++) dst8[q] = (uint8_t)(acc >> (8 * (q & 3)));
                    acc = 0;
                }
                idx++;
            }
            if (idx & 3)
                for (uint32_t q = max(first, idx & ~3u); q < idx; q++) dst8[q] = (uint8_t)(acc >> (8 * (q & 3)));
        }
    }
    __syncthreads();
    return min(tot, count);
}

// block-wide exclusive scan (blockDim.x threads, <= 16 waves); returns the prefix, total in *tot
__device__ inline uint32_t block_xscan(uint32_t v, uint32_t *sh, uint32_t *tot) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += t;
    }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    uint32_t pre = inc - v, all = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t x = sh[w];
        if (w < wv) pre += x;
        all += x;
    }
    __syncthreads();
    *tot = all;
    return pre;
}

struct DBlock;

// ---- status words of an FCX7 decode (fcx_dctx's d7.words, u64 each; host_words mirrors them) ----
constexpr uint32_t kDwTotal = 0;       // decoded bytes (k_dscan_out)
constexpr uint32_t kDwErr = 1;         // error bits (kDErr*), a u32
constexpr uint32_t kDwSymBytes = 2;    // symbol scratch bytes, and right behind them ...
constexpr uint32_t kDwGolombVals = 3;  // ... the golomb values (k_dscan's totals[0..1]): they size the scratch
constexpr uint32_t kDwStats = 4;       // the segment decoder's statistics block (kSs* above)
constexpr uint32_t kDwStored = 12;     // bytes a range decode stored (k_dlz_clip)
constexpr uint32_t kDwWords = 16;      // (128 bytes)
static_assert(kDwStats + kSsWords <= kDwStored && kDwStored < kDwWords, "FCX7 status words");

// The 8-bit Huffman sub-streams of ds[0, nstreams) (nstreams a multiple of 4; unused entries raw with
// count 0): decode tables (k_dtable) and symbols into sym + ds[q].dst (k_dsyms), zeros past a
// stream's end.  A bad tree sets kDErrTree in *err and, when badq is given, lowers *badq to the
// first such stream.  Shared with the FCX8 decoder, whose char streams have this serialisation.
void dec_launch_tables8(const uint8_t *d_in, uint32_t nstreams, const DStream *ds, uint16_t *tbl, uint16_t *child,
                        uint32_t *err, uint32_t *badq, hipStream_t st);
void dec_launch_syms8(const uint8_t *d_in, uint64_t in_len, uint32_t nstreams, const DStream *ds,
                      const uint16_t *tbl, const uint16_t *child, uint8_t *sym, const uint32_t *err,
                      uint64_t *stats, hipStream_t st);

constexpr int kDStages = 5;       // FCX7 stages
constexpr int kD78Stages = 6;     // FCX8 stages (fcx_lz78_dec.hip)

// fcx_lz78_decompress_shard whose messages number the records from rec_base (the stream path's
// groups of a longer run; fcx_lz78_dec.hip)
int lz78_decompress_shard_at(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out,
                             uint64_t cap, uint64_t *out_len, hipStream_t st, uint64_t rec_base);

// ---- the two passes of the range API (fcx_range.hip), per codec; DESIGN.md §9c ----
// Size pass over a run of nblocks records: payload offset and length of every record (the record
// walk) and its decoded size into three device arrays of nblocks entries.  FCX7 decodes the flags
// and the Golomb bytes only; FCX8 runs its stages up to the links and skips the expansion.
int dec7_sizes(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint64_t *d_roff, uint32_t *d_rlen,
               uint32_t *d_dsize, hipStream_t st);
int lz78_sizes(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint64_t *d_roff, uint32_t *d_rlen,
               uint32_t *d_dsize, hipStream_t st);
// Clipped expansion of the nblocks records at d_in (a sub-run: d_in points at its first length
// prefix): the decoded bytes [w.lo, w.hi) of the sub-run go to d_out[0, w.hi - w.lo), nothing else
// is stored.  d_dec_off: the index's nblocks + 1 entries for these records; a record whose decoded
// size is not dec_off[k + 1] - dec_off[k] fails the call.  Messages number the records from rec_base
// (FCX8).  *stored: bytes stored.
int dec7_range(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, const uint64_t *d_dec_off, DClip w,
               uint8_t *d_out, hipStream_t st, uint64_t *stored);
int lz78_range(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, const uint64_t *d_dec_off, DClip w,
               uint8_t *d_out, hipStream_t st, uint64_t rec_base, uint64_t *stored);

// fcx_decompress_range_shard behind its argument checks, for the stream path's groups of a longer
// run: messages number the records from rec_base, *total (when given) = the run's decoded bytes
int range_shard(fcx_dctx *c, char kind, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, const uint64_t *d_rec_off,
                const uint64_t *d_dec_off, uint64_t off, uint64_t len, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                hipStream_t st, uint64_t rec_base, uint64_t *total);

// scratch and counters of the range API (fcx_range.hip)
struct RangeScratch {
    DevBuf<uint64_t> roff, rec_off, dec_off;   // per record (+ 1): the size pass's offsets, the call's own index
    DevBuf<uint32_t> rlen, dsize;
    DevBuf<uint64_t> words;                    // what k_rlocate found
    PinnedBuf<uint64_t> host_words;
    uint64_t stats[FCX_RANGE_STATS] = {};
};

// ---- status words of a verification (fcx_dctx's vf.words, u64 each; host_words mirrors them): the
// first FCX_VERIFY_STATS are the call's stats in the order of fcx.h, written by k_vsummary ----
constexpr uint32_t kVwBlocks = 0;    // records of the run
constexpr uint32_t kVwDiffer = 1;    // blocks that differ
constexpr uint32_t kVwFirst = 2;     // the first of them (preset to ~0: none)
constexpr uint32_t kVwSized = 3;     // blocks whose decoded size is not the block's length
constexpr uint32_t kVwBytes = 4;     // original bytes in differing blocks
constexpr uint32_t kVwDecoded = 5;   // decoded bytes of the run
constexpr uint32_t kVwWords = 8;
static_assert(FCX_VERIFY_STATS <= kVwWords, "verify status words");

// fcx_verify_shard behind its argument checks (fcx_verify.hip), for the stream path's groups of a
// longer file: nblocks may exceed ceil(n / block_bytes) (records the original has no bytes for: they
// differ, with block length 0); messages number the records from rec_base
int verify_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *d_orig,
               uint64_t n, uint32_t block_bytes, uint32_t *d_blocks, uint64_t *stats, hipStream_t st, uint64_t rec_base);

// scratch of the verification (fcx_verify.hip)
struct VerifyScratch {
    DevBuf<uint8_t> buf;             // a group's decoded bytes, grown on demand up to the group bound
    DevBuf<uint32_t> first_diff;     // per record: the first differing byte k_vcompare found
    DevBuf<uint32_t> blocks;         // the stream form's (decoded, first difference) pairs of a group
    DevBuf<uint64_t> words;          // kVw*
    PinnedBuf<uint64_t> host_words;
    uint64_t group_bytes = 0;        // fcx_dctx_set_verify_group (0: 256 MiB)
    uint32_t groups = 0;             // groups of the last call
};

// ---- the run core (fcx_run.hip): what verify_run, repair_apply_run and check_run do
// alike with a device-resident run of records ----
// the checks every entry point over a run and its blocks makes first, `fn` its name in the messages
int run_args(const char *fn, fcx_dctx *c, char kind, const void *d_rec, uint32_t nblocks, uint64_t n, uint32_t block_bytes);
struct RunTimes;
// A run's index: rg.rec_off and rg.dec_off through fcx_index_shard (stage 0 of T), and their copies to
// roff and doff (nblocks + 1 each) issued on st: the caller synchronises before it reads them.
struct RunIndex {
    std::vector<uint64_t> roff, doff;
};
int run_index(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, hipStream_t st, RunTimes &T,
              RunIndex *ix);
// the end of the record group that starts at g0: the bound of fcx_dctx_set_verify_group over doff
uint32_t verify_group_end(const VerifyScratch &V, const uint64_t *doff, uint32_t nblocks, uint32_t g0);
// the run's groups in order, vf.groups set and vf.buf reserved for the largest of them that `staged`
// (records [g0, g1); none given: every group) says goes through the buffer, with `headroom` bytes
// more for a caller that decodes behind the buffer's start (find_run's carry)
struct RunGroup {
    uint32_t g0, g1;
    uint64_t gbytes;   // decoded bytes of its records
};
int run_groups(fcx_dctx *c, const RunIndex &ix, uint32_t nblocks, std::vector<RunGroup> *groups,
               const std::function<bool(uint32_t, uint32_t)> &staged = nullptr, uint64_t headroom = 0);
// records [g0, g0 + nrec) of the run through their codec's decoder to dst, which must give `want` bytes;
// `who` names the entry point in the message, FCX8 messages number the records from rec_base
int decode_group(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, const std::vector<uint64_t> &roff, uint32_t g0,
                 uint32_t nrec, uint8_t *dst, uint64_t want, hipStream_t st, uint64_t rec_base, const char *who);

// ---- status words of a repair call (fcx_dctx's rp.words, u64 each; host_words mirrors them) ----
constexpr uint32_t kRpEntries = 0;     // entries (k_rscan; an apply: the caller's count)
constexpr uint32_t kRpData = 1;        // RAW bytes (k_rscan)
constexpr uint32_t kRpFills = 2;       // FILL entries (k_rscan, k_rmap)
constexpr uint32_t kRpBadEntry = 3;    // an apply: the first entry that fails k_rmap's checks (preset to ~0)
constexpr uint32_t kRpBadRecord = 4;   // ... and the first record without an entry whose size is not its block's
constexpr uint32_t kRpWords = 8;

// fcx_repair_build_shard / fcx_repair_apply_shard behind their argument checks (fcx_repair.hip), for
// the stream path's groups of a longer file: messages number the records from rec_base.  An apply with
// n == kRepairLastFromRun takes the last block's length from the run itself (its entry's from + len,
// or without one its decoded bytes) and reports the n it used in *out_len.
constexpr uint64_t kRepairLastFromRun = ~0ull;
int repair_build_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *d_orig,
                     uint64_t n, uint32_t block_bytes, fcx_repair_entry *d_entries, uint8_t *d_data, uint64_t data_cap,
                     uint32_t *nentries, uint64_t *data_bytes, uint64_t *stats, hipStream_t st, uint64_t rec_base);
int repair_apply_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint64_t n,
                     uint32_t block_bytes, const fcx_repair_entry *d_entries, uint32_t nentries, const uint8_t *d_data,
                     uint64_t data_bytes, uint8_t *d_out, uint64_t cap, uint64_t *out_len, hipStream_t st, uint64_t rec_base);
// The entry map of an apply or a check (fcx_repair.hip): rp.entry_of preset to kNoEntry, k_rmap over the
// entries against rg.dec_off, k_rcheck too when with_check, and the status words on their way to
// rp.host_words.  After the caller's synchronisation entry_map_result turns the first entry or record
// that failed into the call's error (records numbered from rec_base).
int launch_entry_map(fcx_dctx *c, const fcx_repair_entry *d_entries, uint32_t nentries, uint32_t nblocks, uint64_t n,
                     uint32_t block_bytes, uint64_t data_bytes, bool with_check, hipStream_t st);
int entry_map_result(fcx_dctx *c, uint64_t rec_base);

// scratch of the repair calls (fcx_repair.hip); the stream forms' device copies of a group's entries and data
struct RepairScratch {
    DevBuf<uint32_t> pairs;          // verify_run's (decoded, first difference) per record
    DevBuf<fcx_repair_entry> plan;   // k_rplan's entry per record, before the compaction
    DevBuf<uint32_t> entry_of;       // an apply: per record its entry, or ~0
    DevBuf<uint64_t> words;          // kRp*
    PinnedBuf<uint64_t> host_words;
    DevBuf<fcx_repair_entry> entries;
    DevBuf<uint8_t> data;
    uint64_t stats[FCX_REPAIR_STATS] = {};
};

// ---- status words of a check (fcx_dctx's dg.words, u64 each; host_words mirrors them): the first
// FCX_VERIFY_STATS are the call's stats in the order of fcx.h (kVw*), written by k_dgsummary ----
constexpr uint32_t kDgwWords = 8;

// fcx_check_shard behind its argument checks (fcx_digest.hip), for the stream path's groups of a longer
// file: d_crc holds ncrc <= nblocks values, a record from ncrc on has no block and fails with block
// length 0; n: the bytes of the ncrc blocks; messages number the records from rec_base
int check_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint32_t ncrc, uint64_t n,
              uint32_t block_bytes, const fcx_repair_entry *d_entries, uint32_t nentries, const uint8_t *d_data,
              uint64_t data_bytes, const uint32_t *d_crc, uint32_t *d_blocks, uint64_t *stats, hipStream_t st,
              uint64_t rec_base);
// fcx_digest_shard behind its argument checks
int digest_run(fcx_dctx *c, const uint8_t *d_data, uint64_t n, uint32_t block_bytes, uint32_t *d_crc, uint32_t *whole,
               hipStream_t st);

// scratch of the digest calls (fcx_digest.hip); the stream forms' device copies of a shard or a group
struct DigestScratch {
    DevBuf<uint32_t> tables;         // the slicing, folding and power tables (made on the host once)
    DevBuf<uint64_t> seg_at;         // a check: per record two segments, their device addresses ...
    DevBuf<uint32_t> seg_len;        // ... and lengths: the decoded prefix, the RAW bytes
    DevBuf<uint32_t> part;           // their CRC-32
    DevBuf<uint64_t> words;          // kVw*
    PinnedBuf<uint64_t> host_words;
    DevBuf<uint8_t> stage;           // digest_stream: a shard of the original
    DevBuf<uint32_t> crc, blocks;    // the stream forms: a shard's or group's values, a group's pairs
    uint32_t slice = 4;              // fcx_dctx_set_digest_slice
    uint64_t stats[FCX_DIGEST_STATS] = {};
};

// ---- status words of a search (fcx_dctx's fd.words, u64 each; host_words mirrors them) ----
constexpr uint32_t kFwJudged = 0;      // start positions judged (k_fscan)
constexpr uint32_t kFwCand = 1;        // of those, the ones that passed the prefix filter (k_fscan)
constexpr uint32_t kFwHits = 2;        // hits of the call so far: advanced by k_fbase, group by group
constexpr uint32_t kFwGroupBase = 3;   // hits of the call before the group scanned last (k_fbase)
constexpr uint32_t kFwWords = 8;
constexpr uint32_t kFCarry = FCX_FIND_MAX_PATTERN;   // bytes in front of a decoded group: room for the carry

// where a search leaves its hits: the first `cap` of the call at d_hits (device, the shard form), and / or
// every hit through on_hit in order (the stream form, by windows of fd.window hits through fd.hits)
struct FindSink {
    uint64_t *d_hits = nullptr;
    uint64_t cap = 0;
    fcx_hit_fn on_hit = nullptr;
    void *user = nullptr;
};
// fcx_find_shard behind its argument checks (fcx_find.hip), for the stream path's groups of a longer file:
// `base` is the decoded offset of the run's first byte in the file, and the search continues from the
// carry the context holds (fd.carry_len bytes: 0 starts a new search); messages number the records from
// rec_base.  *nhits: the run's hits, *decoded: its decoded bytes.
int find_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint8_t *pattern,
             uint32_t plen, uint64_t base, const FindSink &sink, uint64_t *nhits, uint64_t *decoded, hipStream_t st,
             uint64_t rec_base);

// scratch of the search (fcx_find.hip)
struct FindScratch {
    DevBuf<uint32_t> pat;            // the pattern, zero-padded to kFCarry bytes
    DevBuf<uint8_t> carry;           // kFCarry bytes: the last carry_len decoded bytes seen, right-aligned
    DevBuf<uint16_t> bitmap;         // per tile of 4096 start positions 512 B of hit bits
    DevBuf<uint32_t> tile_count;     // per tile its hits, and ...
    DevBuf<uint32_t> tile_base;      // ... the hits of the group's tiles before it
    DevBuf<uint64_t> hits;           // the stream form's window
    DevBuf<uint64_t> words;          // kFw*
    PinnedBuf<uint64_t> host_words;
    uint32_t carry_len = 0;
    uint32_t window = 0;             // fcx_dctx_set_find_window (0: 1 Mi hits)
    uint64_t stats[FCX_FIND_STATS] = {};
};

// ---- status words of a line call (fcx_dctx's ln.words, u64 each; host_words mirrors them) ----
constexpr uint32_t kLwTotal = 0;       // delimiters of the call so far: advanced by k_lbase, group by group
constexpr uint32_t kLwGroupBase = 1;   // delimiters of the call before the group counted last (k_lbase)
constexpr uint32_t kLwBytes = 2;       // bytes counted (k_lcount)
constexpr uint32_t kLwBadIndex = 3;    // the first offset of a caller's list that is out of order or bound (k_lrank; preset ~0)
constexpr uint32_t kLwSel = 4;         // two words: 1 + the position of each selected delimiter (k_lselect; preset ~0)
constexpr uint32_t kLwLast = 6;        // 1 + the position of the last delimiter seen (k_lcount; 0: none yet)
constexpr uint32_t kLwWords = 8;

// What a line call asks of a run (fcx_lines.hip), and where the run lies in a longer file: the stream forms
// carry the decoded base, the delimiters so far and the last delimiter from group to group.  Offsets,
// ranks and positions are file-wide.
struct LinesReq {
    uint8_t delim = 0x0A;
    uint64_t base = 0;          // decoded offset of the run's first byte in the file
    uint64_t nl_before = 0;     // delimiters before the run
    uint64_t last_before = 0;   // 1 + the position of the last delimiter before the run (0: none)
    bool last_run = true;       // the file ends with this run: an offset equal to its end is ranked
    uint64_t *d_line_off = nullptr;         // the line index: nblocks + 1 values (device), or none
    const uint64_t *d_offsets = nullptr;    // offsets to rank (device, ascending), noff of them, their ...
    uint64_t noff = 0;
    uint64_t *d_lines = nullptr;            // ... line numbers
    bool check_offsets = false;             // order and bound of d_offsets are the caller's: check them
    uint64_t sel[2] = {~0ull, ~0ull};       // the sel[q]-th delimiter of the file (1-based) is to be found; ~0: none
    bool stop_early = false;                // decode no group behind the one that answers both
    // called once the run's decoded bytes are known, before any group: a stream form stages its offsets here
    std::function<int(uint64_t decoded, LinesReq *)> staged;
};
struct LinesRes {
    uint64_t nl = 0;        // delimiters up to the end of what was counted (nl_before included)
    uint64_t last = 0;      // 1 + the position of the last delimiter seen (last_before included)
    uint64_t decoded = 0;   // the run's decoded bytes (the index's)
    uint64_t bad = ~0ull;   // the first bad offset's index
    uint64_t sel[2] = {~0ull, ~0ull};   // 1 + the position of each selected delimiter; ~0: not in what was counted
};
// the line calls behind their argument checks, for the stream path's groups of a longer file: messages
// number the records from rec_base
int lines_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, LinesReq &req, LinesRes *res,
              hipStream_t st, uint64_t rec_base);

// scratch of the line calls (fcx_lines.hip)
struct LinesScratch {
    DevBuf<uint32_t> chunk_count;    // per chunk of kLChunk decoded bytes its delimiters, and ...
    DevBuf<uint32_t> chunk_base;     // ... the delimiters of the group's chunks before it
    DevBuf<uint64_t> words;          // kLw*
    PinnedBuf<uint64_t> host_words;
    DevBuf<uint64_t> offs, lines;    // the stream forms: a group's slice of the offsets and its line numbers
    uint64_t stats[FCX_LINES_CALL_STATS] = {};
};

// ---- status words of a grep (fcx_dctx's gp.words, u64 each; host_words mirrors them).  What travels from group
// to group is in them, never bytes of the open line: positions are run-wide and stored as 1 + position ----
constexpr uint32_t kGwJudged = 0;      // start positions judged (k_gscan)
constexpr uint32_t kGwHits = 1;        // hits (k_gscan)
constexpr uint32_t kGwLines = 2;       // selected lines so far: advanced by k_gbase, group by group
constexpr uint32_t kGwGroupBase = 3;   // selected lines before the group scanned last (k_gbase)
constexpr uint32_t kGwBytes = 4;       // sum of end - start over the selected lines whose end is known
constexpr uint32_t kGwLast = 5;        // 1 + the position of the last delimiter seen (0: none): the open line's start
constexpr uint32_t kGwLastHit = 6;     // 1 + the position of the last hit seen (0: none)
constexpr uint32_t kGwOpen = 7;        // 1: the line open at the group's end is selected: the end of line kGwLines - 1 is to come
constexpr uint32_t kGwClosed = 8;      // the end of the open line the group scanned last closed (0: it closed none)
constexpr uint32_t kGwWords = 16;

// where a grep leaves its lines: the first `cap` of the call at d_start / d_end (device, the shard form), or every
// line through on_line in order (the stream form, by windows of fd.window lines)
struct GrepSink {
    uint64_t *d_start = nullptr, *d_end = nullptr;
    uint64_t cap = 0;
    fcx_range_fn on_line = nullptr;
    void *user = nullptr;
};
// what the stream form keeps between its runs beside the context's words and carry: the decoded offset of the
// next run's first byte, and the start of a selected line that is still open (reported once it closes)
struct GrepCarry {
    uint64_t base = 0;
    bool held = false;
    uint64_t held_start = 0;
};
// fcx_grep_shard behind its argument checks (fcx_grep.hip).  carry == nullptr: a whole run; the line open at its
// end closes at its last byte.  With a carry the run continues the file of the runs before it (carry->base == 0
// starts one), positions are file-wide, and the open line is left to the next run or to the caller.  stats: the
// FCX_GREP_STATS values of the file so far; messages number the records from rec_base.
int grep_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim, const uint8_t *pattern,
             uint32_t plen, const GrepSink &sink, GrepCarry *carry, uint64_t *stats, hipStream_t st, uint64_t rec_base);

// scratch of the grep (fcx_grep.hip); pattern and carry as the search's
struct GrepScratch {
    DevBuf<uint32_t> pat;
    DevBuf<uint8_t> carry;
    DevBuf<uint16_t> hit_bits;       // per tile of 4096 positions 512 B of hit bits (k_gmark: of first hits of a line) ...
    DevBuf<uint16_t> delim_bits;     // ... and 512 B of delimiter bits
    DevBuf<uint32_t> tile_sum;       // per tile 4 words: hits, 1 + first and 1 + last delimiter, 1 + last hit (in the range; 0: none)
    DevBuf<uint64_t> tile_ctx;       // per tile 3 words: 1 + last delimiter and 1 + last hit before it, 1 + first delimiter behind it
    DevBuf<uint32_t> tile_count;     // per tile its first hits, and ...
    DevBuf<uint32_t> tile_base;      // ... those of the group's tiles before it
    DevBuf<uint64_t> words;          // kGw*
    PinnedBuf<uint64_t> host_words;
    DevBuf<uint64_t> win_start, win_end;   // the stream form's window
    uint32_t carry_len = 0;
    uint64_t scratch_bytes = 0;      // device bytes the last call reserved beside the decoded group (bitmaps and tile words)
};

// ---- status words of a multi-range decode (fcx_dctx's rq.words, u64 each; host_words mirrors them) ----
constexpr uint32_t kQwSum = 0;        // bytes of all ranges (k_qchunks)
constexpr uint32_t kQwBadIndex = 1;   // the first range that breaks a rule (k_qlen; preset ~0)
constexpr uint32_t kQwTouched = 2;    // records touched (k_qtouch)
constexpr uint32_t kQwSlice = 4;      // 4 words of the group in work (k_qslice): its ranges [ia, ib), its output span [o_lo, o_hi)
constexpr uint32_t kQwWords = 8;

// fcx_decompress_ranges_shard behind its argument checks (fcx_ranges.hip)
int ranges_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint64_t *d_rec_off,
               const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end, uint64_t nranges, uint8_t *d_out,
               uint64_t cap, uint64_t *out_len, hipStream_t st);

// scratch of the multi-range decode (fcx_ranges.hip); the host forms' device copies of a file and its ranges
struct RangesScratch {
    DevBuf<uint64_t> out_off;        // nranges + 1: the exclusive scan of the range lengths
    DevBuf<uint64_t> chunk_sum;      // per chunk of 1024 ranges its bytes, then the bytes of the chunks before it
    DevBuf<uint8_t> touched;         // per record: does a range hold a byte of it?
    PinnedBuf<uint8_t> host_touched;
    DevBuf<uint64_t> words;          // kQw*
    PinnedBuf<uint64_t> host_words;
    DevBuf<uint8_t> file;            // the host forms: the records
    DevBuf<uint64_t> starts, ends;   // ... and the ranges
    DevBuf<uint8_t> out;
    uint64_t stats[FCX_RANGES_STATS] = {};
};

// ---- pattern sets (fcx_set.hip): its own scan kernel in front of the search's and the grep's
// downstream kernels, which are defined in fcx_find.hip and fcx_grep.hip and launched from fcx_set.hip too ----
__global__ void k_fbase(const uint32_t *__restrict__ tile_count, uint32_t ntiles, uint32_t *__restrict__ tile_base,
                        uint64_t *__restrict__ words);
__global__ void k_fwrite(const uint16_t *__restrict__ bitmap, const uint32_t *__restrict__ tile_count,
                         const uint32_t *__restrict__ tile_base, uint32_t ntiles, const uint64_t *__restrict__ words,
                         uint64_t pos_base, uint64_t win0, uint64_t winlen, uint64_t *__restrict__ out);
__global__ void k_fcarry(const uint8_t *__restrict__ src, uint64_t len, uint32_t keep, uint8_t *__restrict__ carry);
__global__ void k_gtiles(const uint32_t *__restrict__ tile_sum, uint32_t ntiles, uint64_t pos_base, uint64_t *__restrict__ tile_ctx,
                         uint64_t *__restrict__ words, uint64_t *__restrict__ d_end, uint64_t cap);
__global__ void k_gmark(uint16_t *__restrict__ hit_bits, const uint16_t *__restrict__ delim_bits, const uint32_t *__restrict__ tile_sum,
                        const uint64_t *__restrict__ tile_ctx, uint32_t ntiles, uint64_t pos_base, uint32_t *__restrict__ tile_count,
                        uint64_t *__restrict__ words);
__global__ void k_gbase(const uint32_t *__restrict__ tile_count, uint32_t ntiles, uint32_t *__restrict__ tile_base,
                        uint64_t *__restrict__ words);
__global__ void k_gwrite(const uint16_t *__restrict__ hit_bits, const uint16_t *__restrict__ delim_bits,
                         const uint64_t *__restrict__ tile_ctx, const uint32_t *__restrict__ tile_count,
                         const uint32_t *__restrict__ tile_base, uint32_t ntiles, const uint64_t *__restrict__ words,
                         uint64_t pos_base, uint64_t win0, uint64_t winlen, uint64_t *__restrict__ d_start,
                         uint64_t *__restrict__ d_end);
__global__ void k_gfinish(uint64_t *__restrict__ words, uint64_t total, uint64_t *__restrict__ d_end, uint64_t cap);
__global__ void k_gcarry(const uint8_t *__restrict__ src, uint64_t len, uint32_t keep, uint8_t *__restrict__ carry);

// status words of a set scan (fcx_dctx's ps.words, u64 each): the counters of k_sscan, then the 64 per-pattern counts
constexpr uint32_t kSwJudged = 0;      // start positions judged
constexpr uint32_t kSwCand = 1;        // of those, the ones with a non-zero candidate mask
constexpr uint32_t kSwCompares = 2;    // (position, pattern) pairs taken to the full compare
constexpr uint32_t kSwHits = 3;        // positions at which a pattern occurs
constexpr uint32_t kSwCounts = 8;      // FCX_SET_MAX_PATTERNS words: positions at which pattern k occurs
constexpr uint32_t kSwWords = kSwCounts + FCX_SET_MAX_PATTERNS;

// fcx_find_set_shard / fcx_grep_set_shard behind their argument checks (fcx_set.hip), for the stream path's groups
// of a longer file as find_run and grep_run are.  last: the run ends the file, so its last group judges the
// positions that are left with every pattern bounded by the end; without it they stay in the carry, for the next
// run or for set_final.  counts (may be null): the file's per-pattern counts so far.
int find_set_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_pattern_set *set,
                 uint64_t base, const FindSink &sink, bool last, uint64_t *nhits, uint64_t *decoded, uint64_t *counts, hipStream_t st,
                 uint64_t rec_base);
int grep_set_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
                 const fcx_pattern_set *set, const GrepSink &sink, GrepCarry *carry, uint64_t *stats, uint64_t *counts, hipStream_t st,
                 uint64_t rec_base);
// the stream forms' final pass over the carry alone, once the reader has ended at `total` decoded bytes
int find_set_final(fcx_dctx *c, const fcx_pattern_set *set, uint64_t total, const FindSink &sink, uint64_t *nhits, uint64_t *counts,
                   hipStream_t st);
int grep_set_final(fcx_dctx *c, uint8_t delim, const fcx_pattern_set *set, const GrepSink &sink, GrepCarry *carry, uint64_t *stats,
                   uint64_t *counts, hipStream_t st);
// the argument checks the six entry points share; `fn` names the entry point, delim < 0: a find
int set_args(const char *fn, const fcx_pattern_set *set, int delim);

// scratch of the set calls beside the search's (fd) and the grep's (gp), which they use as those do
struct SetScratch {
    DevBuf<uint32_t> block;          // the set's compiled block (fcx_patset.h)
    DevBuf<uint64_t> words;          // kSw*
    PinnedBuf<uint64_t> host_words;
    uint64_t stats[FCX_SET_SCAN_STATS] = {};
};

// ---- context and inverted grep (fcx_context.hip): a select stage in line-number space behind
// k_sscan<true> and k_gtiles.  Status words of a blocks call (fcx_dctx's cx.words, u64 each; host_words mirrors
// them); lines are numbered from 0, "1 + line" words use 0 for none ----
constexpr uint32_t kXwLines = 0;       // delimiters seen so far: the closed lines, and the open line's number
constexpr uint32_t kXwLastBase = 1;    // 1 + the number of the last base line seen (0: none)
constexpr uint32_t kXwBase = 2;        // base lines so far
constexpr uint32_t kXwStarts = 3;      // block starts so far: the blocks
constexpr uint32_t kXwEnds = 4;        // block ends so far (kXwStarts or one less)
constexpr uint32_t kXwSumStart = 5;    // sum of the starts, of the ends, of the first lines, of 1 + the last lines:
constexpr uint32_t kXwSumEnd = 6;      // ... bytes and selected lines are differences of these
constexpr uint32_t kXwSumSLine = 7;
constexpr uint32_t kXwSumELine = 8;
constexpr uint32_t kXwPendEnd = 9;     // the end of line kXwLastBase - 1 + after, closed with no base line behind it
constexpr uint32_t kXwPendLine = 10;   // ... yet (0: none), and that line's number: the open block's end unless a later base line reaches it
constexpr uint32_t kXwGroupS = 11;     // starts and ends before the group's own (k_clines) ...
constexpr uint32_t kXwGroupE = 12;
constexpr uint32_t kXwGroupNS = 13;    // ... and the group's own (k_cscan)
constexpr uint32_t kXwGroupNE = 14;
constexpr uint32_t kXwTotal = 15;      // the run's lines (k_cfinish)
constexpr uint32_t kXwResEnd = 16;     // 3 words each (flag, position, line): the pending end and the pending start
constexpr uint32_t kXwResStart = 19;   // ... that k_clines or k_cfinish resolved, and the end k_cfinish gave the
constexpr uint32_t kXwFinEnd = 22;     // ... block open at the run's end (the stream forms read them)
constexpr uint32_t kXwWords = 32;
constexpr uint32_t kCRing = FCX_GREP_MAX_CONTEXT + 1;   // starts of the last before + 1 lines, by line number mod (before + 1)

// where a blocks call leaves its blocks: the first `cap` at d_start / d_end / d_line (device, the shard form), or
// every block through on_block in order (the stream form, by windows of fd.window)
struct BlockSink {
    uint64_t *d_start = nullptr, *d_end = nullptr, *d_line = nullptr;
    uint64_t cap = 0;
    fcx_block_fn on_block = nullptr;
    void *user = nullptr;
};
// what the stream form keeps between its runs: the decoded offset of the next run's first byte, and the start and
// first line of the block that is still open
struct BlockCarry {
    uint64_t base = 0;
    bool held = false;
    uint64_t held_start = 0, held_line = 0;
};
// fcx_grep_blocks_shard behind its argument checks (fcx_context.hip), shaped as grep_set_run and grep_set_final
int blocks_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, uint8_t delim,
               const fcx_pattern_set *set, const fcx_grep_opts &opts, const BlockSink &sink, BlockCarry *carry, uint64_t *stats,
               uint64_t *counts, hipStream_t st, uint64_t rec_base);
int blocks_final(fcx_dctx *c, uint8_t delim, const fcx_pattern_set *set, const fcx_grep_opts &opts, const BlockSink &sink,
                 BlockCarry *carry, uint64_t *stats, uint64_t *counts, hipStream_t st);
// the argument checks the three entry points share
int blocks_args(const char *fn, const fcx_pattern_set *set, uint8_t delim, const fcx_grep_opts *opts);
// what fcx_set.hip does for the blocks calls: its scratch and the set's block made ready, the grep's tile scratch,
// k_sscan<true> over one range (*ntiles: its tiles), and the set's counters fetched and published
int context_ready(fcx_dctx *c, const fcx_pattern_set *set, bool fresh, hipStream_t st);
int context_reserve(fcx_dctx *c, uint64_t range_bytes);
int context_scan(fcx_dctx *c, const fcx_pattern_set *set, uint8_t delim, const uint8_t *src, uint64_t len, bool final,
                 uint32_t *ntiles, hipStream_t st);
int context_fetch(fcx_dctx *c, hipStream_t st);
void context_publish(fcx_dctx *c, const fcx_pattern_set *set, uint64_t *counts);

// scratch of the blocks calls beside the grep's (gp) and the set's (ps)
struct ContextScratch {
    DevBuf<uint16_t> base_bits;      // per tile 512 B each: the delimiters that end a base line, ...
    DevBuf<uint16_t> start_bits;     // ... those behind which a block starts, ...
    DevBuf<uint16_t> end_bits;       // ... and those that end a block
    DevBuf<uint32_t> tile_cs;        // per tile 4 words: delimiters, base lines, its first base line, 1 + its last (tile-local)
    DevBuf<uint64_t> tile_lctx;      // per tile 3 words: its first line, 1 + the last base line before it, the first behind it
    DevBuf<uint32_t> tile_cnt;       // per tile its block starts and ends, and ...
    DevBuf<uint32_t> tile_rank;      // ... those of the group's tiles before it
    DevBuf<uint64_t> ring;           // kCRing line starts
    DevBuf<uint64_t> words;          // kXw*
    PinnedBuf<uint64_t> host_words;
    DevBuf<uint64_t> win[4];         // the stream form's window: starts, first lines, ends, last lines
    DevBuf<uint64_t> lines;          // the host form's first lines
    uint64_t grep_bytes = 0, extra_bytes = 0;   // what the call reserved of the grep's scratch and beside it
};

// what the select kernels write through: the first cap blocks of a call
struct CxOut {
    uint64_t *d_start, *d_end, *d_line;
    uint64_t cap;
};

// ---- regular-expression grep (fcx_regex.hip): its own scan stage (k_rmap, k_rentry, k_rmark) in front
// of k_gtiles and the select stage of fcx_context.hip, whose kernels and host helpers it launches and calls as they
// are ----
__global__ void k_cbase(const uint16_t *__restrict__ hit_bits, const uint16_t *__restrict__ delim_bits,
                        const uint32_t *__restrict__ tile_sum, const uint64_t *__restrict__ gctx, uint32_t ntiles, uint64_t pos_base,
                        uint32_t invert, uint16_t *__restrict__ base_bits, uint32_t *__restrict__ tile_cs);
__global__ void k_clines(const uint32_t *__restrict__ tile_cs, uint32_t ntiles, uint32_t before, uint32_t after,
                         uint64_t *__restrict__ tile_lctx, uint64_t *__restrict__ words, const uint64_t *__restrict__ ring, CxOut out);
__global__ void k_cmark(const uint16_t *__restrict__ delim_bits, const uint16_t *__restrict__ base_bits,
                        const uint32_t *__restrict__ tile_cs, const uint64_t *__restrict__ tile_lctx, uint32_t ntiles, uint64_t pos_base,
                        uint32_t before, uint32_t after, uint16_t *__restrict__ start_bits, uint16_t *__restrict__ end_bits,
                        uint32_t *__restrict__ tile_cnt, uint64_t *__restrict__ words, uint64_t *__restrict__ ring);
__global__ void k_cscan(const uint32_t *__restrict__ tile_cnt, uint32_t ntiles, uint32_t *__restrict__ tile_rank,
                        uint64_t *__restrict__ words);
__global__ void k_cwrite(const uint16_t *__restrict__ delim_bits, const uint16_t *__restrict__ start_bits,
                         const uint16_t *__restrict__ end_bits, const uint32_t *__restrict__ tile_cnt,
                         const uint32_t *__restrict__ tile_rank, const uint64_t *__restrict__ tile_lctx, uint32_t ntiles,
                         const uint64_t *__restrict__ words, uint64_t pos_base, uint32_t local, uint64_t win_s, uint64_t win_e,
                         uint64_t winlen, uint64_t *__restrict__ o_start, uint64_t *__restrict__ o_line, uint64_t *__restrict__ o_end,
                         uint64_t *__restrict__ o_eline);
__global__ void k_cfinish(uint64_t *__restrict__ words, const uint64_t *__restrict__ gwords, const uint64_t *__restrict__ ring,
                          uint32_t before, uint32_t after, uint32_t invert, uint64_t total, CxOut out);
int ready_context(fcx_dctx *c);
int reserve_context_tiles(fcx_dctx *c, uint64_t range_bytes);
CxOut out_of(const BlockSink &sink);
void host_close(const BlockSink &sink, BlockCarry *carry, uint64_t end, uint64_t eline);
void host_open(BlockCarry *carry, uint64_t start, uint64_t line);
void host_resolved(const BlockSink &sink, BlockCarry *carry, const uint64_t *hw);
void blocks_stats_out(fcx_dctx *c, uint64_t total, uint64_t *stats);

// fcx_grep_regex_blocks_shard behind its argument checks, shaped as blocks_run and blocks_final
int regex_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_regex *re,
              const fcx_grep_opts &opts, const BlockSink &sink, BlockCarry *carry, uint64_t *stats, hipStream_t st, uint64_t rec_base);
int regex_final(fcx_dctx *c, const fcx_regex *re, const fcx_grep_opts &opts, const BlockSink &sink, BlockCarry *carry, uint64_t *stats,
                hipStream_t st);
// the argument checks the three entry points share
int regex_args(const char *fn, const fcx_regex *re, const fcx_grep_opts *opts);

// scratch of the regex calls beside the grep's (gp) and the blocks calls' (cx)
struct RegexScratch {
    DevBuf<uint8_t> block;           // the compiled regex (fcx_regex.h)
    DevBuf<uint8_t> tile_map;        // per tile the map state -> state of its positions, `states` bytes each
    DevBuf<uint8_t> tile_entry;      // per tile the state in front of its first position
    DevBuf<uint32_t> state;          // the state in front of the next range's first judged position
    uint64_t tile_bytes = 0;         // what the call reserved of the two tile arrays (part of fcx_dctx_grep_scratch)
    uint64_t stats[FCX_REGEX_SCAN_STATS] = {};
};

// ---- cut (fcx_cut.hip).  Status words of a cut (fcx_dctx's ct.words, u64 each; host_words mirrors
// them): what travels from group to group is in them ----
constexpr uint32_t kKwOut = 0;         // output bytes of the call so far: advanced by k_kbase, group by group
constexpr uint32_t kKwGroupBase = 1;   // output bytes before the range cut last (k_kbase)
constexpr uint32_t kKwJudged = 2;      // bytes judged (k_kmark)
constexpr uint32_t kKwDelims = 3;      // delimiters seen
constexpr uint32_t kKwSeps = 4;        // separators seen
constexpr uint32_t kKwSepsKept = 5;    // ... and kept
constexpr uint32_t kKwTicks = 6;       // the saturated tick count of the line open at the end of the range cut last (k_kentry)
constexpr uint32_t kKwWords = 8;

// the cut calls behind their argument checks (fcx_cut.hip): *out_len the output's total, stats the FCX_CUT_STATS
// values (may be null); messages of cut_run number the records from rec_base.  cont: the run continues the text of
// the cut_run calls before it (the stream form's groups of a longer file): the open line's ticks and the counters
// go on from the context's words, the output starts at d_out[0] again and *out_len, stats[0] and stats[5] are this
// run's alone.
int cut_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const fcx_cut *cut, uint8_t *d_out,
            uint64_t cap, uint64_t *out_len, uint64_t *stats, hipStream_t st, uint64_t rec_base, bool cont);
int cut_ranges_run(fcx_dctx *c, char kind, const uint8_t *d_rec, uint64_t rec_len, uint32_t nblocks, const uint64_t *d_rec_off,
                   const uint64_t *d_dec_off, const uint64_t *d_start, const uint64_t *d_end, uint64_t nranges, const fcx_cut *cut,
                   uint8_t *d_out, uint64_t cap, uint64_t *out_len, uint64_t *stats, hipStream_t st);

// scratch of the cut calls (fcx_cut.hip)
struct CutScratch {
    DevBuf<uint32_t> sel;            // the cut's selection table (fcx_cut.h)
    DevBuf<uint16_t> keep_bits;      // per tile of 4096 bytes 512 B of keep bits, in hit_bits' layout
    DevBuf<uint32_t> tile_sum;       // per tile its summary: bit 31 it holds a delimiter, the ticks behind the last (or all)
    DevBuf<uint32_t> tile_entry;     // per tile the open line's ticks at its first byte
    DevBuf<uint32_t> tile_count;     // per tile its kept bytes, and ...
    DevBuf<uint32_t> tile_base;      // ... those of the range's tiles before it
    DevBuf<uint64_t> words;          // kKw*
    PinnedBuf<uint64_t> host_words;
    DevBuf<uint8_t> gathered;        // the ranges form: the concatenation of the ranges' bytes
    DevBuf<uint8_t> out;             // the host form's output
    uint64_t scratch_bytes = 0;      // device bytes the last call reserved beside the decoded group
    uint64_t stats[FCX_CUT_STATS] = {};
};

// FCX7 scratch (fcx_dec.hip): per block, dropped as a whole when a call has more blocks ...
struct Dec7Blocks {
    uint32_t cap_blocks = 0;
    DevBuf<DBlock> blk;
    DevBuf<DStream> ds, ds_sel;   // (ds_sel: the size pass's list of the flags and Golomb-byte streams)
    DevBuf<uint64_t> symb;
    DevBuf<uint16_t> tbl, child;
};
// ... and per decoded symbol, each grown when a call needs more; the status words (kDw*)
struct Dec7 : Dec7Blocks {
    DevBuf<uint8_t> sym;
    DevBuf<uint32_t> glen;
    DevBuf<uint64_t> words;
    PinnedBuf<uint64_t> host_words;
};
// FCX8 scratch (fcx_lz78_dec.hip), made by the first FCX8 call
struct Scratch78;
void free_scratch78(Scratch78 *s);

}  // namespace fcx

// the decoder context of include/fcx.h
struct fcx_dctx {
    int device = 0;
    bool profiling = false;
    fcx::Dec7 d7;
    std::unique_ptr<fcx::Scratch78, fcx::Calls<fcx::free_scratch78>> d78;
    fcx::RangeScratch rg;
    fcx::VerifyScratch vf;
    fcx::RepairScratch rp;
    fcx::DigestScratch dg;
    fcx::FindScratch fd;
    fcx::LinesScratch ln;
    fcx::GrepScratch gp;
    fcx::RangesScratch rq;
    fcx::SetScratch ps;
    fcx::ContextScratch cx;
    fcx::RegexScratch rx;
    fcx::CutScratch ct;
    // the last call's stages: FCX7 read on the first fcx_dctx_stage query, FCX8 summed over its batches
    fcx::StageTimes times{fcx::kD78Stages};
};

namespace fcx {

// the stage times of a call over a run: events only when the context profiles; publish() makes the
// call's own table the context's (it replaces the last inner decode's)
struct RunTimes {
    std::unique_ptr<StageTimes> T;
    hipStream_t st;
    RunTimes(fcx_dctx *c, int stages, hipStream_t s) : T(c->profiling ? new StageTimes(stages) : nullptr), st(s) {}
    void mark(int i) {
        if (T) T->mark(i, st);
    }
    int add(int first, int last) { return T ? T->add(first, last) : FCX_OK; }
    void publish(fcx_dctx *c, const char *const *names, int n) {
        c->times.reset();
        if (!T) return;
        for (int i = 0; i < n; i++) c->times.ms[i] = T->ms[i];
        c->times.publish(names, n);
    }
};

}  // namespace fcx

#endif  // FCX_DEC_SHARED_H
