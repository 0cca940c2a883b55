// fcx_lz78_dec.hip — GPU decoder of FCX8 / LZ78 block records (gfx950).
//
// Replaces my_decompress_file_lz78 (my_compress.cpp:3478-3710) with its callees
// huffman_decode_idxGroup (3009-3054), huffman_decode_char (930-984) and my_LZ78_decompress
// (1901-1934) for a device-resident run of block records ([u32 len][payload]..., the file
// minus its 10-byte header).  A phrase is the chars on the path from its trie root down to its
// token, so once every token knows its parent token the block decodes token-parallel:
//
//   k78d_index    one thread walks the record lengths (a sequential chain of u32s);
//   per batch of <= kBatch records (scratch is per token of the batch in flight):
//   k78d_head     workgroup per record: wcnt, the used-index bitmap's length (popcount scan to
//                 the wcnt-th set bit), G, tree, N, W, in-group positions, char header; bounds;
//   k78d_scan     token / index offsets of the batch's records, the char streams' descriptors;
//   k78d_pindex   workgroup per record: pindex[i] = position of the bitmap's i-th set bit
//                 (popcount per lane, scan, scatter);
//   k78d_gtable   workgroup per record: the group tree ((lc, rc) u32 pairs, root G-2) checked
//                 (one parent per node, every node reaches the root within 32 steps) and turned
//                 into the wide lookup table of fcx_dec_shared.h; the char trees go through the
//                 FCX7 decoder's k_dtable (same serialisation);
//   k78d_groups   workgroup per record: group ids u16[N] with the segment decoder; the chars
//                 u8[N] come from the FCX7 decoder's k_dsyms;
//   k78d_links    workgroup per record: r = g*256 + gpos -> ix = pindex[r] -> parent token
//                 ix - 1; phrase length = ancestors + 1 (bounded walk); scan -> phrase starts,
//                 block length, the tail-zero rule (3701-3703);
//   k78d_scan_out output offsets of the records, capacity check;
//   k78d_expand   lane per token: its char at the phrase's last byte, its ancestors' chars
//                 before it, at most kLong bytes; a longer phrase notes its kLong-th ancestor;
//   k78d_expand_long  wave per long phrase: the rest of it is the last-kLong windows of its
//                 kLong-th, 2 kLong-th, ... ancestors, copied 64 bytes at a time.
//
// Everything is written straight to its final place in the caller's buffer.
//
// The range API (fcx_range.hip) runs the same batches with another last step
// (Pass78): the size pass hands the sizes out behind k78d_scan_out and expands nothing; the range
// decode checks the sizes against the index and expands with k78d_expand_clip /
// k78d_expand_long_clip, which store only the bytes of the window.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_dec_shared.h"

namespace fcx78d {
using namespace fcx;

constexpr uint32_t kBatch = 256;                                // records decoded per batch
constexpr uint32_t kCapBlock = FCX_MAX_BLOCK_BYTES + 8;         // decoded bytes / tokens of one record
constexpr uint32_t kGmax = FCX_MAX_BLOCK_BYTES / 256 + 4;       // groups of a <= 1 MiB block
constexpr uint32_t kLong = 64;                                  // phrase bytes one lane writes
// A token of depth d has d - 1 ancestors of depths 1..d-1, all phrases of the block: d (d + 1) / 2
// <= kCapBlock, so a deeper chain belongs to a record whose decoded size is past the limit.
constexpr uint32_t kMaxDepth = 1449;
static_assert((uint64_t)kMaxDepth * (kMaxDepth + 1) / 2 > kCapBlock, "depth bound");
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct DRec {
    uint64_t off;   // payload byte offset in the input
    uint64_t out;   // output byte offset
    uint32_t tok;   // first token slot of the record in the batch's token arrays (4-aligned)
    uint32_t pix;   // first pindex entry
    uint32_t len, wcnt, nbm, G, N, Wg, ts, nw;
    uint32_t o_tree, o_gw, o_gpos, o_cpairs, o_cw;
    uint32_t out_len, ok, pad;
};

// ---- status words of an FCX8 decode (Scratch78's words, u64 each; host_words mirrors them) ----
constexpr uint32_t kW8Total = 0;       // running output bytes (k78d_scan_out)
constexpr uint32_t kW8Err = 1;         // error bits (kDErr*), a u32
constexpr uint32_t kW8Tokens = 2;      // token slots of the batch (k78d_scan): they size the scratch, as do ...
constexpr uint32_t kW8Pindex = 3;      // ... its pindex entries
constexpr uint32_t kW8BadRec = 4;      // first bad record (1-based, u32; kNone: none)
constexpr uint32_t kW8BadStream = 5;   // first bad char stream of the batch (u32; kNone: none)
constexpr uint32_t kW8Stats = 8;       // the segment decoder's statistics block (kSs*, fcx_dec_shared.h)
constexpr uint32_t kW8Stored = 16;     // bytes a range decode stored (the clipped expansion)
constexpr uint32_t kWords = 32;
static_assert(kW8BadStream == kW8BadRec + 1 && kW8Stats + kSsWords <= kW8Stored && kW8Stored < kWords,
              "FCX8 status words");

// the error word as one value for the whole workgroup (lanes that read it apart could part at a barrier)
__device__ inline bool wg_err(const uint32_t *err) { return __syncthreads_or(threadIdx.x == 0 && *err != 0); }

__global__ void k78d_index(const uint8_t *in, uint64_t in_len, uint32_t nblocks, uint64_t *roff, uint32_t *rlen,
                           uint32_t *err, uint32_t *badrec) {
    uint64_t off = 0;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (off + 4 > in_len || ld_u32le(in, off) > in_len - off - 4) {
            atomicOr(err, kDErrRecord);
            atomicMin(badrec, b + 1);
            return;
        }
        const uint32_t len = ld_u32le(in, off);
        roff[b] = off + 4;
        rlen[b] = len;
        off += 4 + (uint64_t)len;
    }
}

// workgroup per record: the payload header (my_decompress_file_lz78 3478-3600)
__global__ __launch_bounds__(256) void k78d_head(const uint8_t *in, const uint64_t *roff, const uint32_t *rlen,
                                                 DRec *rec, uint32_t r0, uint32_t *err, uint32_t *badrec) {
    __shared__ uint32_t sh[4];
    __shared__ uint32_t s_last;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (wg_err(err)) return;   // (a broken record chain leaves roff / rlen unset)
    const uint8_t *p = in + roff[b];
    const uint32_t len = rlen[b];
    bool ok = len >= 4;
    const uint32_t wcnt = ok ? ld_u32le(p, 0) : 0u;
    ok = ok && wcnt != 0 && wcnt <= kCapBlock + 2;   // wcnt == 0: the reference reads pIndex[-1] (3502)
    // the bitmap ends with the byte of its wcnt-th set bit: popcount scan over 4 KiB pieces
    if (tid == 0) s_last = kNone;
    __syncthreads();
    if (ok) {
        // (a bitmap of a valid block is <= kCapBlock / 8 + 1 bytes; the scan's own limit keeps its
        // 32-bit positions exact)
        const uint32_t avail = min(len - 4, 1u << 28);
        const uint8_t *bm = p + 4;
        uint32_t seen = 0;
        bool found = false;
        for (uint32_t c0 = 0; c0 < avail && !found; c0 += 256 * 16) {
            const uint32_t lo = c0 + 16 * tid;
            uint32_t pc = 0;
            for (uint32_t k = 0; k < 16; k++)
                if (lo + k < avail) pc += (uint32_t)__builtin_popcount(bm[lo + k]);
            uint32_t tot;
            const uint32_t pre = seen + block_xscan(pc, sh, &tot);
            if (pre < wcnt && wcnt <= pre + pc) {   // this lane's bytes hold the wcnt-th set bit
                uint32_t need = wcnt - pre;
                for (uint32_t k = 0; k < 16 && lo + k < avail; k++) {
                    uint32_t x = bm[lo + k];
                    const uint32_t c = (uint32_t)__builtin_popcount(x);
                    if (need <= c) {
                        for (uint32_t i = 1; i < need; i++) x &= x - 1;
                        s_last = 8 * (lo + k) + (uint32_t)__ffs(x) - 1;
                        break;
                    }
                    need -= c;
                }
            }
            seen += tot;
            __syncthreads();
            found = s_last != kNone;
        }
        ok = found;
    }
    if (tid != 0) return;
    DRec R{};
    R.off = roff[b];
    R.len = len;
    uint64_t q = 4;
    auto room = [&](uint64_t n) {
        if ((uint64_t)len - q < n) ok = false;
        return ok;
    };
    uint32_t G = 0, N = 0, W = 0;
    if (ok) {
        R.wcnt = wcnt;
        R.nbm = s_last / 8 + 1;
        q += R.nbm;   // (inside the record: the bit was found there)
        if (room(4)) {
            G = ld_u32le(p, q);
            q += 4;
        }
    }
    if (ok) {
        if (G > 1) {
            if (G > kGmax || !room(8ull * (G - 1) + 8)) ok = false;
            else {
                R.o_tree = (uint32_t)q;
                q += 8ull * (G - 1);
                N = ld_u32le(p, q);
                W = ld_u32le(p, q + 4);
                q += 8;
                if (room(4ull * W)) {
                    R.o_gw = (uint32_t)q;
                    q += 4ull * W;
                }
            }
        } else if (room(4)) {
            N = ld_u32le(p, q);
            q += 4;
        }
    }
    if (ok && (N > kCapBlock || !room(N))) ok = false;
    if (ok) {
        R.o_gpos = (uint32_t)q;
        q += N;
        // char sub-stream header (huffman_decode_char 930-984, my_huffman_decode_char 1107-1187)
        if (room(1)) {
            const uint32_t ts = p[q], nbm2 = (2 * ts + 7) / 8, hdr = 1 + nbm2 + 2 * ts;
            if (room((uint64_t)hdr + 4)) {
                const uint32_t nw = ld_u32le(p, q + hdr);
                if (room((uint64_t)hdr + 4 + 4ull * nw)) {
                    R.ts = ts;
                    R.o_cpairs = (uint32_t)(q + 1 + nbm2);
                    R.o_cw = (uint32_t)(q + hdr + 4);
                    R.nw = min(nw, N);   // a code is <= 32 bits: N symbols never read past N words
                }
            }
        }
    }
    if (ok) {
        R.G = G;
        R.N = N;
        R.Wg = min(W, N);
        R.ok = 1;
    } else {
        R.wcnt = 0;
        atomicOr(err, kDErrHeader);
        atomicMin(badrec, r0 + b + 1);
    }
    rec[b] = R;
}

// token and index offsets of the batch's records (nb <= kBatch = the workgroup), the descriptors
// of their char streams (nds of them, a multiple of 4) for the FCX7 decoder's table and symbol kernels
__global__ __launch_bounds__(kBatch) void k78d_scan(uint32_t nb, DRec *rec, DStream *ds, uint32_t nds,
                                                    uint64_t *words) {
    __shared__ uint32_t sh[kBatch / 64];
    const uint32_t b = threadIdx.x;
    const bool live = b < nb && rec[b].ok;
    const uint32_t n4 = live ? (rec[b].N + 3) & ~3u : 0u, wc = live ? rec[b].wcnt : 0u;
    uint32_t tt, tp;
    const uint32_t tok = block_xscan(n4, sh, &tt);
    const uint32_t pix = block_xscan(wc, sh, &tp);
    if (b < nb) {
        rec[b].tok = tok;
        rec[b].pix = pix;
    }
    if (b < nds) {
        DStream s{};
        s.raw = 1;
        if (live) {
            const DRec R = rec[b];
            s.words_bit = 8 * (R.off + R.o_cw);
            s.pairs_off = R.off + R.o_cpairs;
            s.dst = tok;
            s.nbits = 32 * R.nw;
            s.count = R.N;
            s.ts = R.ts;
            s.raw = 0;
        }
        ds[b] = s;
    }
    if (b == 0) {
        words[kW8Tokens] = tt;
        words[kW8Pindex] = tp;
    }
}

// workgroup per record: pindex[i] = position of the i-th set bit of the bitmap (3494-3500)
__global__ __launch_bounds__(1024) void k78d_pindex(const uint8_t *in, const DRec *rec, uint32_t *pindex,
                                                    const uint32_t *err) {
    __shared__ uint32_t sh[16];
    if (wg_err(err)) return;
    const DRec R = rec[blockIdx.x];
    if (!R.ok) return;
    const uint32_t tid = threadIdx.x;
    const uint8_t *bm = in + R.off + 4;
    uint32_t *pi = pindex + R.pix;
    uint32_t seen = 0;
    for (uint32_t c0 = 0; c0 < R.nbm; c0 += 1024 * 16) {
        const uint32_t lo = c0 + 16 * tid;
        uint32_t x[16], pc = 0;
        for (uint32_t k = 0; k < 16; k++) {
            x[k] = lo + k < R.nbm ? bm[lo + k] : 0u;
            pc += (uint32_t)__builtin_popcount(x[k]);
        }
        uint32_t tot;
        uint32_t rank = seen + block_xscan(pc, sh, &tot);
        for (uint32_t k = 0; k < 16; k++)
            for (uint32_t v = x[k]; v && rank < R.wcnt; v &= v - 1) pi[rank++] = 8 * (lo + k) + (uint32_t)__ffs(v) - 1;
        seen += tot;
    }
}

// workgroup per record with a group tree: huffman_decode_idxGroup's tree (3009-3054) as the wide
// lookup table.  G - 1 nodes of (lc, rc) u32 pairs, root = node G - 2; a child < G is a leaf, else
// child - G is a node.  Valid: every node but the root has exactly one parent and reaches the root
// within 32 steps (so the links are a tree and every code is <= 32 bits).
__global__ __launch_bounds__(256) void k78d_gtable(const uint8_t *in, const DRec *rec, uint32_t r0, uint32_t *gtbl,
                                                   uint16_t *gchild, uint32_t *err, uint32_t *badrec) {
    __shared__ uint16_t ch[2 * kGmax];
    __shared__ uint32_t par[kGmax];    // parent node | side << 15; kNone = none
    __shared__ uint32_t code[kGmax];
    __shared__ uint8_t dep[kGmax];
    __shared__ uint32_t bad;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (wg_err(err)) return;
    const DRec R = rec[b];
    if (!R.ok || R.G <= 1 || R.N == 0) return;
    const uint32_t G = R.G, nodes = G - 1, root = G - 2;
    const uint8_t *p = in + R.off;
    if (tid == 0) bad = 0;
    for (uint32_t k = tid; k < nodes; k += 256) par[k] = kNone;
    __syncthreads();
    for (uint32_t x = tid; x < 2 * nodes; x += 256) {   // pair j = (lc, rc) at o_tree + 8 j
        uint32_t v = ld_u32le(p, R.o_tree + 4ull * x);
        if (v >= G) {
            const uint32_t k = v - G;
            if (k >= nodes) { bad = 1; v = 0; }
            else v = kWideNode | k;
        }
        ch[x] = (uint16_t)v;
    }
    __syncthreads();
    for (uint32_t x = tid; x < 2 * nodes; x += 256)
        if (ch[x] & kWideNode)
            if (atomicCAS(&par[ch[x] & 0x7FFFu], kNone, (x >> 1) | ((x & 1) << 15)) != kNone) bad = 1;   // two parents
    __syncthreads();
    if (tid == 0 && par[root] != kNone) bad = 1;   // the root is nobody's child
    for (uint32_t k = tid; k < nodes; k += 256) {
        // gathered leaf-up, the branch at depth i ends in bit i (root first, LSB-first)
        uint32_t d = 0, cd = 0, n = k;
        while (n != root) {
            const uint32_t pv = par[n];
            if (pv == kNone || d >= 31) { bad = 1; break; }
            cd = (cd << 1) | (pv >> 15);
            n = pv & 0x7FFFu;
            d++;
        }
        dep[k] = (uint8_t)d;
        code[k] = cd;
    }
    __syncthreads();
    uint32_t *T = gtbl + 1024ull * b;
    uint16_t *C = gchild + 2ull * kGmax * b;
    for (uint32_t x = tid; x < 1024; x += 256) T[x] = kNone;
    for (uint32_t x = tid; x < 2 * nodes; x += 256) C[x] = ch[x];
    __syncthreads();
    for (uint32_t x = tid; x < 2 * nodes; x += 256) {
        const uint32_t node = x >> 1, side = x & 1;
        const uint32_t d = dep[node] + 1u;
        const uint32_t cd = code[node] | (side << dep[node]);
        if (!(ch[x] & kWideNode)) {
            if (d <= kDTblBits) {
                const uint32_t e = ch[x] | (d << 16);
                for (uint32_t sfx = 0; sfx < (1u << (kDTblBits - d)); sfx++) T[cd | (sfx << d)] = e;
            }
        } else if (d == kDTblBits) {
            T[cd] = 0x80000000u | (ch[x] & 0x7FFFu);
        }
    }
    __syncthreads();
    if (tid == 0 && bad) {
        atomicOr(err, kDErrTree);
        atomicMin(badrec, r0 + b + 1);
    }
}

// workgroup per record: the N group ids (u16).  G <= 1: no group stream, every token in group 0;
// ids the words do not cover stay 0 (the reference's calloc).
__global__ __launch_bounds__(kDSymThreads) void k78d_groups(const uint8_t *in, uint64_t in_len, const DRec *rec,
                                                            const uint32_t *gtbl, const uint16_t *gchild,
                                                            uint16_t *grp, const uint32_t *err, uint64_t *stats) {
    __shared__ uint32_t T[1u << kDTblBits];
    __shared__ uint16_t C[2 * kGmax];
    __shared__ uint32_t st[kDSymThreads + 1];
    __shared__ uint32_t cnt[kDSymThreads / 64];
    __shared__ uint32_t flag[2];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (wg_err(err)) return;
    const DRec R = rec[b];
    if (!R.ok || R.N == 0) return;
    uint16_t *g = grp + R.tok;
    uint32_t got = 0;
    if (R.G > 1) {
        for (uint32_t x = tid; x < (1u << kDTblBits); x += kDSymThreads) T[x] = gtbl[1024ull * b + x];
        for (uint32_t x = tid; x < 2 * (R.G - 1); x += kDSymThreads) C[x] = gchild[2ull * kGmax * b + x];
        __syncthreads();
        uint64_t bit0;
        const BitBuf src = make_bits(in, in_len, bit0);
        got = seg_decode<kCodeHuffWide>(src, bit0 + 8 * (R.off + R.o_gw), 32 * R.Wg, R.N, (const uint16_t *)T, C,
                                        nullptr, (uint32_t *)g, st, cnt, flag, stats);
    }
    for (uint32_t x = got + tid; x < R.N; x += kDSymThreads) g[x] = 0;
}

// workgroup per record: parent links, phrase lengths, phrase starts (3586-3595, my_LZ78_decompress
// 1901-1934).  par[t] = ix (0: no parent, else parent token ix - 1 < t); pstart has N + 1 entries.
constexpr uint32_t kLinkTPT = 4;
__global__ __launch_bounds__(1024) void k78d_links(const uint8_t *in, DRec *rec, uint32_t r0, const uint32_t *pindex,
                                                   const uint16_t *grp, const uint8_t *chr, uint32_t *par,
                                                   uint32_t *pstart, uint32_t *err, uint32_t *badrec) {
    __shared__ uint32_t sh[16];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (wg_err(err)) return;
    const DRec R = rec[b];
    if (!R.ok) return;
    const uint32_t N = R.N;
    const uint8_t *gp = in + R.off + R.o_gpos;
    const uint16_t *g = grp + R.tok;
    const uint32_t *pi = pindex + R.pix;
    uint32_t *pa = par + R.tok;
    uint32_t *ps = pstart + R.tok + b;
    bool bad = false;
    for (uint32_t t = tid; t < N; t += 1024) {
        const uint32_t r = (uint32_t)g[t] * 256u + gp[t];
        uint32_t ix = 0;
        if (r >= R.wcnt) bad = true;
        else {
            ix = pi[r];
            if (ix > t) { bad = true; ix = 0; }
        }
        pa[t] = ix;
    }
    bad = __syncthreads_or(bad);   // (also: every link is in place before the walks)
    uint32_t run = 0;
    for (uint32_t c0 = 0; c0 < N && !bad; c0 += 1024 * kLinkTPT) {
        uint32_t d[kLinkTPT], sum = 0;
        bool deep = false;
        for (uint32_t u = 0; u < kLinkTPT; u++) {
            const uint32_t t = c0 + kLinkTPT * tid + u;
            d[u] = 0;
            if (t < N) {
                uint32_t a = t, n = 1, ix;
                while ((ix = pa[a]) != 0 && n <= kMaxDepth) {   // ix - 1 < a: the chain descends
                    a = ix - 1;
                    n++;
                }
                deep = deep || n > kMaxDepth;
                d[u] = n;
                sum += n;
            }
        }
        uint32_t tot;
        uint32_t pre = run + block_xscan(sum, sh, &tot);
        for (uint32_t u = 0; u < kLinkTPT; u++) {
            const uint32_t t = c0 + kLinkTPT * tid + u;
            if (t < N) ps[t] = pre;
            pre += d[u];
        }
        run += tot;   // (<= 4096 kMaxDepth + kCapBlock)
        bad = __syncthreads_or(deep || run > kCapBlock);   // decoded size past the reference's buffer
    }
    if (tid != 0) return;
    if (bad) {
        atomicOr(err, kDErrDist);
        atomicMin(badrec, r0 + b + 1);
        rec[b].out_len = 0;
        return;
    }
    ps[N] = run;
    // a block whose decoded bytes end in 0x00 loses that byte (3701-3703); the last byte is the last token's char
    rec[b].out_len = run - ((N > 0 && chr[R.tok + N - 1] == 0) ? 1u : 0u);
}

// output offsets of the batch's records behind the bytes of the batches before; capacity check
__global__ __launch_bounds__(kBatch) void k78d_scan_out(uint32_t nb, DRec *rec, uint64_t cap, uint64_t *words,
                                                        uint32_t *err) {
    __shared__ uint64_t off[kBatch];
    const uint32_t b = threadIdx.x;
    off[b] = b < nb ? rec[b].out_len : 0;
    __syncthreads();
    if (b == 0) {
        uint64_t o = words[kW8Total];
        for (uint32_t i = 0; i < nb; i++) {
            const uint64_t l = off[i];
            off[i] = o;
            o += l;
        }
        words[kW8Total] = o;
        if (o > cap) atomicOr(err, kDErrOutCap);
    }
    __syncthreads();
    if (b < nb) rec[b].out = off[b];
}

// lane per token: the last min(L, kLong) bytes of its phrase, walking up its ancestors; a longer
// phrase leaves its kLong-th ancestor in skip[] for k78d_expand_long.  grid (x, record).
__global__ __launch_bounds__(256) void k78d_expand(const DRec *rec, const uint8_t *chr, const uint32_t *par,
                                                   const uint32_t *pstart, uint32_t *skip, uint8_t *out,
                                                   const uint32_t *err) {
    const uint32_t b = blockIdx.y;
    const DRec R = rec[b];
    if (*err || !R.ok) return;
    const uint8_t *c = chr + R.tok;
    const uint32_t *pa = par + R.tok;
    const uint32_t *ps = pstart + R.tok + b;
    uint8_t *o = out + R.out;
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < R.N; t += gridDim.x * 256) {
        const uint32_t e = ps[t + 1], L = e - ps[t];
        const uint32_t steps = min(L, kLong);
        uint32_t a = t;
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t pos = e - 1 - k;
            if (pos < R.out_len) o[pos] = c[a];   // (the dropped tail zero is not written)
            if (k + 1 < L) a = pa[a] - 1;
        }
        if (L > kLong) skip[R.tok + t] = a;
    }
}

// wave per long phrase: bytes [0, L - kLong) are the last-kLong windows of its kLong-th,
// 2 kLong-th, ... ancestors, which k78d_expand has written; <= kMaxDepth / kLong hops.
__global__ __launch_bounds__(256) void k78d_expand_long(const DRec *rec, const uint32_t *pstart, const uint32_t *skip,
                                                        uint8_t *out, const uint32_t *err) {
    const uint32_t b = blockIdx.y;
    const DRec R = rec[b];
    if (*err || !R.ok) return;
    const uint32_t *ps = pstart + R.tok + b;
    const uint32_t *sk = skip + R.tok;
    uint8_t *o = out + R.out;
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (uint32_t base = wave * 64; base < R.N; base += nwaves * 64) {
        const uint32_t t = base + lane;
        const uint32_t e = t < R.N ? ps[t + 1] : 0u, L = t < R.N ? e - ps[t] : 0u;
        uint64_t mask = __ballot(L > kLong);
        while (mask) {
            const int j = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            uint32_t rem = (uint32_t)__shfl((int)L, j, 64) - kLong;
            uint32_t dend = (uint32_t)__shfl((int)e, j, 64) - 1 - kLong;   // last byte still to write
            uint32_t a = sk[base + j];
            while (rem > 0) {   // a: the ancestor of depth rem
                const uint32_t n = min(rem, kLong);
                const uint32_t send = ps[a + 1] - 1;
                if (lane < n) o[dend - lane] = o[send - lane];
                rem -= n;
                dend -= n;
                if (rem > 0) a = sk[a];
            }
        }
    }
}

// ---- the range API's passes (fcx_range.hip) ----
// the size pass: the batch's decoded sizes as a plain array
__global__ __launch_bounds__(kBatch) void k78d_sizes_out(uint32_t nb, const DRec *rec, uint32_t *dsize) {
    const uint32_t b = threadIdx.x;
    if (b < nb) dsize[b] = rec[b].out_len;
}

// the batch's decoded sizes against the index's (dec_off: the batch's first entry)
__global__ __launch_bounds__(kBatch) void k78d_check_sizes(uint32_t nb, const DRec *rec, uint32_t r0,
                                                           const uint64_t *dec_off, uint32_t *err, uint32_t *badrec) {
    const uint32_t b = threadIdx.x;
    if (b >= nb || *err) return;
    if (dec_off[b + 1] - dec_off[b] != (uint64_t)rec[b].out_len) {
        atomicOr(err, kDErrIndex);
        atomicMin(badrec, r0 + b + 1);
    }
}

// A record's part of the window: its bytes [clo, chi) are stored, byte x at out[ob0 + x].
struct Clip78 {
    uint32_t clo, chi;
    int64_t ob0;
    __device__ bool set(const DRec &R, const DClip &w) {   // false: the record is outside the window
        if (R.out >= w.hi || R.out + R.out_len <= w.lo) return false;
        clo = w.lo > R.out ? (uint32_t)(w.lo - R.out) : 0u;
        chi = (uint32_t)min((uint64_t)R.out_len, w.hi - R.out);   // (<= out_len: the dropped tail zero stays out)
        ob0 = (int64_t)R.out - (int64_t)w.lo;
        return true;
    }
};

__device__ inline void wave_count(uint32_t n, unsigned long long *stored) {   // every lane of the wave calls
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(stored, (unsigned long long)n);
}

// k78d_expand clipped: a token whose phrase misses the window stores nothing and, when its phrase
// is short, is not walked at all; a long phrase still leaves its kLong-th ancestor in skip[], which
// the long phrases below it hop over.  The first and last phrase of the window are cut byte-wise.
__global__ __launch_bounds__(256) void k78d_expand_clip(const DRec *rec, const uint8_t *chr, const uint32_t *par,
                                                        const uint32_t *pstart, uint32_t *skip, uint8_t *out,
                                                        const uint32_t *err, DClip w, unsigned long long *stored) {
    const uint32_t b = blockIdx.y;
    const DRec R = rec[b];
    Clip78 cl;
    if (*err || !R.ok || !cl.set(R, w)) return;
    const uint8_t *c = chr + R.tok;
    const uint32_t *pa = par + R.tok;
    const uint32_t *ps = pstart + R.tok + b;
    uint32_t n = 0;
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < R.N; t += gridDim.x * 256) {
        const uint32_t s = ps[t], e = ps[t + 1], L = e - s;
        const bool hit = s < cl.chi && e > cl.clo;
        if (!hit && L <= kLong) continue;
        const uint32_t steps = min(L, kLong);
        uint32_t a = t;
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t pos = e - 1 - k;
            if (hit && pos >= cl.clo && pos < cl.chi) {
                out[cl.ob0 + pos] = c[a];
                n++;
            }
            if (k + 1 < L) a = pa[a] - 1;
        }
        if (L > kLong) skip[R.tok + t] = a;
    }
    wave_count(n, stored);
}

// k78d_expand_long clipped: the ancestors' bytes may lie outside the window, so a piece is not
// copied from the output: lane i of a piece walks i links up from the piece's ancestor and stores
// that token's char.  Pieces outside the window are hopped over.
__global__ __launch_bounds__(256) void k78d_expand_long_clip(const DRec *rec, const uint8_t *chr, const uint32_t *par,
                                                             const uint32_t *pstart, const uint32_t *skip, uint8_t *out,
                                                             const uint32_t *err, DClip w, unsigned long long *stored) {
    const uint32_t b = blockIdx.y;
    const DRec R = rec[b];
    Clip78 cl;
    if (*err || !R.ok || !cl.set(R, w)) return;
    const uint8_t *c = chr + R.tok;
    const uint32_t *pa = par + R.tok;
    const uint32_t *ps = pstart + R.tok + b;
    const uint32_t *sk = skip + R.tok;
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    uint32_t cnt = 0;
    for (uint32_t base = wave * 64; base < R.N; base += nwaves * 64) {
        const uint32_t t = base + lane;
        const uint32_t s = t < R.N ? ps[t] : 0u, e = t < R.N ? ps[t + 1] : 0u, L = e - s;
        // the bytes before the last kLong: [s, e - kLong)
        uint64_t mask = __ballot(L > kLong && s < cl.chi && e - kLong > cl.clo);
        while (mask) {
            const int j = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            uint32_t rem = (uint32_t)__shfl((int)L, j, 64) - kLong;
            uint32_t dend = (uint32_t)__shfl((int)e, j, 64) - 1 - kLong;   // last byte still to write
            uint32_t a = sk[base + j];
            while (rem > 0) {   // a: the ancestor of depth rem; this piece: bytes (dend - n, dend]
                const uint32_t n = min(rem, kLong);
                const uint32_t pos = dend - lane;
                if (lane < n && pos >= cl.clo && pos < cl.chi) {
                    uint32_t x = a;
                    for (uint32_t i = 0; i < lane; i++) x = pa[x] - 1;   // (depth rem > lane: the chain holds)
                    out[cl.ob0 + pos] = c[x];
                    cnt++;
                }
                rem -= n;
                if (rem == 0 || dend - n < cl.clo) break;   // the rest lies before the window
                dend -= n;
                a = sk[a];
            }
        }
    }
    wave_count(cnt, stored);
}

}  // namespace fcx78d

// ---------------------------------------------------------------------------
namespace fcx {
using namespace fcx78d;

struct Scratch78 {
    DevBuf<uint64_t> roff;          // per record of the call
    DevBuf<uint32_t> rlen;
    DevBuf<DRec> rec;               // kBatch
    DevBuf<DStream> ds;             // kBatch
    DevBuf<uint16_t> ctbl, cchild;  // char tables, kBatch x (1024, 512)
    DevBuf<uint32_t> gtbl;          // kBatch x 1024
    DevBuf<uint16_t> gchild;        // kBatch x 2 kGmax
    DevBuf<uint64_t> words;         // the status words (kW8*)
    PinnedBuf<uint64_t> host_words; // (made last: set = the fixed-size parts above are)
    DevBuf<uint8_t> chr;            // per token slot of the largest batch so far: 1 B
    DevBuf<uint16_t> grp;           //                 2 B
    DevBuf<uint32_t> par, pstart, skip;   // 3 x 4 B (pstart: + 1 per record)
    DevBuf<uint32_t> pindex;        // per used index of the largest batch so far: 4 B
};
void free_scratch78(Scratch78 *s) { delete s; }

static const char *kD78StageNames[] = {"header", "index", "tables", "symbols", "links", "expand"};
static_assert(sizeof(kD78StageNames) / sizeof(kD78StageNames[0]) == kD78Stages, "FCX8 stage names");

// n elements and the slack the kernels' wide loads may touch
template <typename T>
static int grow(DevBuf<T> &b, uint64_t n, const char *what) { return b.reserve(n * sizeof(T) + 64, what); }

static int verdict(const Scratch78 *S, uint64_t rec_base, uint32_t batch0) {
    const uint32_t e = (uint32_t)S->host_words[kW8Err];
    if (!e) return FCX_OK;
    if (e & ~kDErrOutCap) {
        uint64_t k = (uint32_t)S->host_words[kW8BadRec];
        if (e == kDErrIndex)
            return fail(FCX_ERR_FORMAT, "fcx_lz78: the index disagrees with the run at record " + std::to_string(rec_base + k));
        const uint32_t q = (uint32_t)S->host_words[kW8BadStream];   // a char tree: its stream's place in the batch
        if (q != kNone) k = std::min<uint64_t>(k, (uint64_t)batch0 + q + 1);
        return fail(FCX_ERR_FORMAT, "fcx_lz78: malformed record " + std::to_string(rec_base + k));
    }
    return fail(FCX_ERR_CAPACITY, "fcx_lz78: decoded output exceeds capacity");
}

// What a run does with a batch once its links and sizes are known: the expansion (pass == nullptr,
// the full decode), or one of the range API's passes.
struct Pass78 {
    uint32_t *dsize = nullptr;           // size pass: the decoded sizes go here, nothing is expanded
    const uint64_t *dec_off = nullptr;   // range decode: the index's entries for these records, and ...
    DClip w;                             // ... the window the clipped expansion stores
};

static int lz78_run(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out, uint64_t cap,
                    uint64_t *out_len, hipStream_t st, uint64_t rec_base, const Pass78 *pass) {
    FCX_HIP(hipSetDevice(c->device));
    StageTimes &T = c->times;
    T.reset();
    *out_len = 0;
    if (nblocks == 0) return FCX_OK;
    if (!c->d78) c->d78.reset(new Scratch78());
    Scratch78 *S = c->d78.get();
    if (!S->host_words) {
        FCX_TRY(grow(S->rec, kBatch, "records"));
        FCX_TRY(grow(S->ds, kBatch, "streams"));
        FCX_TRY(grow(S->ctbl, 1024ull * kBatch, "char tables"));
        FCX_TRY(grow(S->cchild, 512ull * kBatch, "char trees"));
        FCX_TRY(grow(S->gtbl, 1024ull * kBatch, "group tables"));
        FCX_TRY(grow(S->gchild, 2ull * kGmax * kBatch, "group trees"));
        FCX_TRY(grow(S->words, kWords, "words"));
        FCX_HIP(S->host_words.alloc(8 * kWords));
    }
    FCX_TRY(grow(S->roff, nblocks, "record offsets"));
    FCX_TRY(grow(S->rlen, nblocks, "record lengths"));
    const uint64_t *hw = S->host_words;
    uint32_t *err = (uint32_t *)(S->words + kW8Err), *badrec = (uint32_t *)(S->words + kW8BadRec),
             *badq = (uint32_t *)(S->words + kW8BadStream);
    uint64_t *stats = S->words + kW8Stats;
    FCX_HIP(hipMemsetAsync(S->words, 0, 8 * kWords, st));
    FCX_HIP(hipMemsetAsync(badrec, 0xFF, 16, st));   // (kW8BadRec and kW8BadStream: kNone)
    const bool prof = c->profiling;
    auto mark = [&](int i) { if (prof) T.mark(i, st); };
    mark(0);
    hipLaunchKernelGGL(k78d_index, dim3(1), dim3(1), 0, st, d_in, in_len, nblocks, S->roff, S->rlen, err, badrec);
    for (uint32_t r0 = 0; r0 < nblocks; r0 += kBatch) {
        const uint32_t nb = std::min(kBatch, nblocks - r0), nds = (nb + 3) & ~3u;
        if (r0) mark(0);
        hipLaunchKernelGGL(k78d_head, dim3(nb), dim3(256), 0, st, d_in, S->roff + r0, S->rlen + r0, S->rec, r0, err, badrec);
        hipLaunchKernelGGL(k78d_scan, dim3(1), dim3(kBatch), 0, st, nb, S->rec, S->ds, nds, S->words);
        mark(1);
        // the batch's token and index counts size the scratch; the error bits of the batch before
        FCX_HIP(hipMemcpyAsync(S->host_words, S->words, 8 * kWords, hipMemcpyDeviceToHost, st));
        FCX_HIP(hipStreamSynchronize(st));
        FCX_TRY(verdict(S, rec_base, r0 ? r0 - kBatch : 0));
        if (prof) FCX_TRY(T.add(0, 1));
        const uint64_t ntok = hw[kW8Tokens], npix = hw[kW8Pindex];
        FCX_TRY(grow(S->chr, ntok, "chars"));
        FCX_TRY(grow(S->grp, ntok, "groups"));
        FCX_TRY(grow(S->par, ntok, "parents"));
        FCX_TRY(grow(S->pstart, ntok + kBatch, "phrase starts"));
        FCX_TRY(grow(S->skip, ntok, "skips"));
        FCX_TRY(grow(S->pindex, npix, "index table"));
        if (r0) FCX_HIP(hipMemsetAsync(badq, 0xFF, 8, st));   // (the batch before had no bad char tree)
        mark(1);
        hipLaunchKernelGGL(k78d_pindex, dim3(nb), dim3(1024), 0, st, d_in, S->rec, S->pindex, err);
        mark(2);
        hipLaunchKernelGGL(k78d_gtable, dim3(nb), dim3(256), 0, st, d_in, S->rec, r0, S->gtbl, S->gchild, err, badrec);
        dec_launch_tables8(d_in, nds, S->ds, S->ctbl, S->cchild, err, badq, st);
        mark(3);
        dec_launch_syms8(d_in, in_len, nds, S->ds, S->ctbl, S->cchild, S->chr, err, stats, st);
        hipLaunchKernelGGL(k78d_groups, dim3(nb), dim3(kDSymThreads), 0, st, d_in, in_len, S->rec, S->gtbl, S->gchild,
                           S->grp, err, stats);
        mark(4);
        hipLaunchKernelGGL(k78d_links, dim3(nb), dim3(1024), 0, st, d_in, S->rec, r0, S->pindex, S->grp, S->chr, S->par,
                           S->pstart, err, badrec);
        hipLaunchKernelGGL(k78d_scan_out, dim3(1), dim3(kBatch), 0, st, nb, S->rec, cap, S->words, err);
        mark(5);
        if (!pass) {
            hipLaunchKernelGGL(k78d_expand, dim3(32, nb), dim3(256), 0, st, S->rec, S->chr, S->par, S->pstart, S->skip, d_out,
                               err);
            hipLaunchKernelGGL(k78d_expand_long, dim3(8, nb), dim3(256), 0, st, S->rec, S->pstart, S->skip, d_out, err);
        } else if (pass->dsize) {
            hipLaunchKernelGGL(k78d_sizes_out, dim3(1), dim3(kBatch), 0, st, nb, S->rec, pass->dsize + r0);
        } else {
            unsigned long long *stored = (unsigned long long *)(S->words + kW8Stored);
            hipLaunchKernelGGL(k78d_check_sizes, dim3(1), dim3(kBatch), 0, st, nb, S->rec, r0, pass->dec_off + r0, err, badrec);
            hipLaunchKernelGGL(k78d_expand_clip, dim3(32, nb), dim3(256), 0, st, S->rec, S->chr, S->par, S->pstart, S->skip,
                               d_out, err, pass->w, stored);
            hipLaunchKernelGGL(k78d_expand_long_clip, dim3(8, nb), dim3(256), 0, st, S->rec, S->chr, S->par, S->pstart,
                               S->skip, d_out, err, pass->w, stored);
        }
        mark(6);
        FCX_HIP(hipGetLastError());
        if (prof) FCX_TRY(T.add(1, kD78Stages));
    }
    FCX_HIP(hipMemcpyAsync(S->host_words, S->words, 8 * kWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    FCX_TRY(verdict(S, rec_base, (nblocks - 1) / kBatch * kBatch));
    if (prof) T.publish(kD78StageNames, kD78Stages);
    *out_len = hw[kW8Total];
    return FCX_OK;
}

int lz78_decompress_shard_at(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out,
                             uint64_t cap, uint64_t *out_len, hipStream_t st, uint64_t rec_base) {
    return lz78_run(c, d_in, in_len, nblocks, d_out, cap, out_len, st, rec_base, nullptr);
}

int lz78_sizes(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint64_t *d_roff, uint32_t *d_rlen,
               uint32_t *d_dsize, hipStream_t st) {
    Pass78 pass;
    pass.dsize = d_dsize;
    uint64_t total = 0;
    FCX_TRY(lz78_run(c, d_in, in_len, nblocks, nullptr, ~0ull, &total, st, 0, &pass));
    if (nblocks) {   // the record walk's offsets and lengths (k78d_index)
        FCX_HIP(hipMemcpyAsync(d_roff, c->d78->roff, 8ull * nblocks, hipMemcpyDeviceToDevice, st));
        FCX_HIP(hipMemcpyAsync(d_rlen, c->d78->rlen, 4ull * nblocks, hipMemcpyDeviceToDevice, st));
    }
    return FCX_OK;
}

int lz78_range(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, const uint64_t *d_dec_off, DClip w,
               uint8_t *d_out, hipStream_t st, uint64_t rec_base, uint64_t *stored) {
    Pass78 pass;
    pass.dec_off = d_dec_off;
    pass.w = w;
    uint64_t total = 0;
    FCX_TRY(lz78_run(c, d_in, in_len, nblocks, d_out, ~0ull, &total, st, rec_base, &pass));
    *stored = nblocks ? c->d78->host_words[kW8Stored] : 0;
    return FCX_OK;
}
}  // namespace fcx

using namespace fcx;

namespace {
// fcx_lz78_decompress_block / _host: a decoder context per host thread on the current device
thread_local std::unique_ptr<fcx_dctx, Calls<fcx_dctx_destroy>> g_dctx;

int thread_dctx(fcx_dctx **out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(FCX_ERR_HIP, "no HIP device: the GPU decoder needs one");
    if (g_dctx && g_dctx->device != dev) {
        g_dctx.reset();
        (void)hipSetDevice(dev);
    }
    if (!g_dctx) {
        fcx_dctx *c = nullptr;
        FCX_TRY(fcx_dctx_create(&c, dev));
        g_dctx.reset(c);
    }
    *out = g_dctx.get();
    return FCX_OK;
}
}  // namespace

extern "C" {

uint32_t fcx_lz78_decode_batch_records(void) { return kBatch; }

int fcx_lz78_decompress_shard(fcx_dctx *ctx, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out,
                              uint64_t cap, uint64_t *out_len, void *stream) {
    if (!ctx || !d_in || !d_out || !out_len) return fail(FCX_ERR_ARG, "fcx_lz78_decompress_shard: NULL argument");
    return lz78_decompress_shard_at(ctx, d_in, in_len, nblocks, d_out, cap, out_len, (hipStream_t)stream, 0);
}

int64_t fcx_lz78_decompress_block(const uint8_t *in, uint32_t len, uint8_t *out, uint64_t cap) {
    if (!in || !out) return fail(FCX_ERR_ARG, "fcx_lz78_decompress_block: NULL argument");
    fcx_dctx *c = nullptr;
    FCX_TRY(thread_dctx(&c));
    const uint64_t dcap = std::min<uint64_t>(cap, kCapBlock);
    DevBuf<uint8_t> din, dout;
    FCX_HIP(din.alloc(4ull + len));
    FCX_HIP(dout.alloc(dcap + 16));
    FCX_HIP(hipMemcpy(din, &len, 4, hipMemcpyHostToDevice));
    FCX_HIP(hipMemcpy(din + 4, in, len, hipMemcpyHostToDevice));
    uint64_t n = 0;
    FCX_TRY(fcx_lz78_decompress_shard(c, din, 4ull + len, 1, dout, dcap, &n, nullptr));
    FCX_HIP(hipMemcpy(out, dout, n, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

int fcx_lz78_decompress_host(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len) {
    if (!in || !out_len || (cap && !out)) return fail(FCX_ERR_ARG, "fcx_lz78_decompress_host: NULL argument");
    // header check as main() (4140-4159): "FCX" magic, anything but '7' selects LZ78
    if (in_len < FCX_HEADER_BYTES || memcmp(in, "FCX", 3) != 0 || in[3] == '7')
        return fail(FCX_ERR_FORMAT, "fcx_lz78_decompress_host: not an FCX8 (LZ78) stream");
    *out_len = 0;
    uint16_t nblk;
    memcpy(&nblk, in + 8, 2);
    uint64_t q = FCX_HEADER_BYTES;
    for (uint32_t b = 0; b < nblk; b++) {
        if (q + 4 > in_len) return fail(FCX_ERR_FORMAT, "fcx_lz78: truncated record length");
        uint32_t sz;
        memcpy(&sz, in + q, 4);
        q += 4;
        if (q + sz > in_len) return fail(FCX_ERR_FORMAT, "fcx_lz78: truncated record");
        q += sz;
    }
    // bytes after the block_num counted records are ignored, as main() does (4162-4201: it reads
    // block_num records and judges the result by size).  The u16 count wraps past 65535
    // blocks (:105), so such a file decodes to its counted blocks and the CLI reports FAIL
    // on the size, like the reference.
    if (nblk == 0) return FCX_OK;
    fcx_dctx *c = nullptr;
    FCX_TRY(thread_dctx(&c));
    uint8_t scratch = 0;
    return fcx_decompress_host(c, in, q, cap ? out : &scratch, cap, out_len);
}

}  // extern "C"

