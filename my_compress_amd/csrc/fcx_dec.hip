// fcx_dec.hip — GPU decoder of FCX7 / LZ77 block records (gfx950).
//
// Replaces my_decompress_file_lz77 (my_compress.cpp:2255-2393) with its callees
// my_huffman_decode_char (1107-1187), golomb_rice_decode (309-358),
// decombine_bits (1315-1338) and my_LZ77_decompress (1716-1735), for a whole
// device-resident run of block records ([u32 len][payload]..., the file minus
// its 10-byte header).  The decoded bytes equal the reference decoder's,
// including its quirks: a single-symbol Huffman sub-stream (ts = 0, W = 0)
// decodes as zeros, symbols the words run out of stay zero, and the block stops
// at the first match token it has no (p, l) for (2331-2335).
//
//   k_dindex  one thread walks the record lengths (a sequential chain of u32s);
//   k_dhead   one thread per block parses the payload header: N, the four
//             sub-stream headers (tree, W, words), pCnt, G; bounds-checked;
//   k_dscan   block offsets of the decoded symbols, golomb values and tokens;
//   k_dtable  one wave per sub-stream: parent links from the serialized tree,
//             codes (root->leaf paths, LSB-first) and a 1024-entry lookup table
//             (codes <= 10 bits resolve in one probe, longer ones continue from
//             their depth-10 node);
//   k_dsyms   one workgroup per sub-stream: the bit stream is cut into 1024-bit
//             segments, one per lane; lanes agree on each segment's first code
//             boundary by a Jacobi fixed point (Huffman codes resynchronise
//             within a few symbols), scan their symbol counts and decode again
//             into place.  The same machinery decodes the Golomb-Rice lengths;
//   k_dlen    one workgroup per block: the early-stop token, sum of lengths =
//             decoded block size; k_dscan_out: output offsets;
//   k_dlz     one workgroup per block walks its tokens in steps: each step takes
//             the tokens whose output fits an LDS tile, scatters literal bytes
//             and copy links (x -> x - p), and resolves the links by pointer
//             jumping against the tile and the 2 KiB history before it.
//
// The range API (fcx_range.hip) runs two more passes over the same kernels: the size
// pass (dec7_sizes) decodes only the flags and the Golomb bytes (k_dhead and k_dscan give only those
// room in the symbol scratch, k_dsel lists their descriptors for k_dtable and k_dsyms), stops behind
// k_dlen and hands the sizes out (k_dsizes_out); the range decode (dec7_range) runs every stage on a
// sub-run, checks the sizes against the index (k_dcheck_sizes) and expands with k_dlz_clip, k_dlz's
// body with a clip window.
//
// The bit reader, the table probes, the segment decoder and the block scan are in
// fcx_dec_shared.h, which the FCX8 decoder (fcx_lz78_dec.hip) includes as well; it also
// runs k_dtable and k_dsyms on its char streams (dec_launch_tables8 / dec_launch_syms8).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_device.h"
#include "fcx_dec_shared.h"

namespace fcx {

constexpr uint32_t kDLzThreads = 1024;
constexpr uint32_t kDLzTile = 8192;              // output bytes resolved per LDS step
constexpr uint32_t kDLzTPT = 4;                  // tokens read per lane and step
constexpr uint32_t kMaxTokensPerBlock = FCX_MAX_BLOCK_BYTES;

struct DBlock {
    uint64_t payload_off;   // byte offset of the payload in the input
    uint64_t sym_off;       // symbol scratch: [flags nb][chars N][P bytes][golomb 4G], 4-aligned parts
    uint64_t glen_off;      // index of this block's first golomb value
    uint64_t out_off;       // output byte offset
    uint32_t payload_len;
    uint32_t N, pcnt, G, nb, pbytes;
    uint32_t n_eff, pc_eff; // tokens decoded (early stop) and matches among them
    uint32_t out_len;
    uint32_t glen_got;      // golomb values decoded
    uint32_t pad[2];
};

// ---------------------------------------------------------------------------
__global__ void k_dindex(const uint8_t *in, uint64_t in_len, uint32_t nblocks, DBlock *blk, uint32_t *err) {
    uint64_t off = 0;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (off + 4 > in_len) { atomicOr(err, kDErrRecord); return; }
        const uint32_t len = ld_u32le(in, off);
        if (len > in_len - off - 4) { atomicOr(err, kDErrRecord); return; }
        blk[b].payload_off = off + 4;
        blk[b].payload_len = len;
        off += 4 + (uint64_t)len;
    }
}

struct HCursor {
    const uint8_t *in;
    uint64_t p, end;
    bool ok;
    __device__ uint32_t u32() {
        if (p + 4 > end) { ok = false; return 0; }
        const uint32_t v = ld_u32le(in, p);
        p += 4;
        return v;
    }
    __device__ uint64_t take(uint64_t n) {
        if (n > end - p) { ok = false; return p; }
        const uint64_t q = p;
        p += n;
        return q;
    }
};

__device__ bool parse_sub(HCursor &c, DStream &s, uint32_t count) {
    const uint64_t tsb = c.take(1);
    if (!c.ok) return false;
    const uint32_t ts = c.in[tsb];
    const uint32_t nbm = (2 * ts + 7) / 8;
    c.take(nbm);
    s.pairs_off = c.take(2ull * ts);
    const uint32_t W = c.u32();
    const uint64_t wo = c.take(4ull * W);
    if (!c.ok || W > (1u << 26)) return false;
    s.words_bit = 8 * wo;
    s.nbits = 32 * W;
    s.ts = ts;
    s.count = count;
    s.raw = 0;
    s.rawv = 0;
    return true;
}

// one thread per block: payload header (my_decompress_file_lz77 2255-2330)
// smask (kAllStreams, kSizeStreams): the sub-streams that get room in the symbol scratch
__global__ void k_dhead(const uint8_t *in, uint32_t nblocks, DBlock *blk, DStream *ds, uint64_t *symb,
                        uint32_t smask, uint32_t *err) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    if (*err & kDErrRecord) return;
    DBlock &B = blk[b];
    HCursor c{in, B.payload_off, B.payload_off + B.payload_len, true};
    DStream *s = ds + 4ull * b;
    const uint32_t N = c.u32();
    bool ok = c.ok && N <= kMaxTokensPerBlock;
    const uint32_t nb = (N + 7) / 8;
    if (ok) {
        if (nb > 1) ok = parse_sub(c, s[0], nb);
        else {
            const uint64_t r = c.take(nb);
            s[0] = DStream{};
            s[0].raw = 1;
            s[0].count = nb;
            s[0].rawv = (c.ok && nb) ? c.in[r] : 0u;
            ok = c.ok;
        }
    }
    if (ok) ok = parse_sub(c, s[1], N);
    uint32_t pcnt = 0, pbytes = 0, G = 0;
    if (ok) {
        pcnt = c.u32();
        ok = c.ok && pcnt <= N;
    }
    if (ok) {
        pbytes = (kPBits * pcnt) / 8 + 1;   // :2311
        ok = parse_sub(c, s[2], pbytes);
    }
    if (ok) {
        G = c.u32();
        // a Golomb code is <= 67 bits (l <= 257): more words than that cannot be valid
        ok = c.ok && (uint64_t)G <= (67ull * pcnt + 31) / 32 + 1;
    }
    if (ok) {
        if (G > 0) ok = parse_sub(c, s[3], 4 * G);
        else { s[3] = DStream{}; s[3].count = 0; s[3].raw = 1; }
    }
    if (!ok) {
        atomicOr(err, kDErrHeader);
        B.N = B.nb = B.pcnt = B.G = B.pbytes = 0;
        for (int q = 0; q < 4; q++) { s[q] = DStream{}; s[q].raw = 1; }
        symb[b] = 0;
        return;
    }
    B.N = N; B.nb = nb; B.pcnt = pcnt; B.G = G; B.pbytes = pbytes;
    auto a4 = [](uint64_t x) { return (x + 3) & ~3ull; };
    symb[b] = (smask & 1u ? a4(nb) : 0) + (smask & 2u ? a4(N) : 0) + (smask & 4u ? a4(pbytes) : 0) +
              (smask & 8u ? 4ull * G : 0);
}

// exclusive scans over blocks (one workgroup, sequential chunks): symbol bytes,
// golomb values; sets DStream.dst and DBlock.sym_off / glen_off; totals out
__global__ void k_dscan(uint32_t nblocks, DBlock *blk, DStream *ds, const uint64_t *symb, uint32_t smask,
                        uint64_t *totals) {
    __shared__ uint64_t sh[2][1024 / 64];
    __shared__ uint64_t carry[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { carry[0] = 0; carry[1] = 0; }
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nblocks; b0 += blockDim.x) {
        const uint32_t b = b0 + tid;
        uint64_t v[2] = {b < nblocks ? symb[b] : 0, b < nblocks ? (uint64_t)blk[b].pcnt : 0};
        uint64_t inc[2];
        for (int q = 0; q < 2; q++) {
            inc[q] = v[q];
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t t = __shfl_up(inc[q], o, 64);
                if (lane >= (uint32_t)o) inc[q] += t;
            }
            if (lane == 63) sh[q][wv] = inc[q];
        }
        __syncthreads();
        uint64_t pre[2], tot[2];
        for (int q = 0; q < 2; q++) {
            uint64_t p = 0, a = 0;
            for (uint32_t w = 0; w < blockDim.x / 64; w++) {
                if (w < wv) p += sh[q][w];
                a += sh[q][w];
            }
            pre[q] = carry[q] + p + inc[q] - v[q];
            tot[q] = a;
        }
        if (b < nblocks) {
            DBlock &B = blk[b];
            B.sym_off = pre[0];
            B.glen_off = pre[1];
            auto a4 = [](uint64_t x) { return (x + 3) & ~3ull; };
            DStream *s = ds + 4ull * b;
            s[0].dst = pre[0];   // (a sub-stream outside smask has no room: it is not decoded)
            s[1].dst = s[0].dst + (smask & 1u ? a4(B.nb) : 0);
            s[2].dst = s[1].dst + (smask & 2u ? a4(B.N) : 0);
            s[3].dst = s[2].dst + (smask & 4u ? a4(B.pbytes) : 0);
        }
        __syncthreads();
        if (tid == 0) { carry[0] += tot[0]; carry[1] += tot[1]; }
        __syncthreads();
    }
    if (tid == 0) { totals[0] = carry[0]; totals[1] = carry[1]; }   // (kDwSymBytes, kDwGolombVals) the host sizes the scratch from these
}

// ---------------------------------------------------------------------------
// decode tables: one wave per (block, stream) with a tree.
// tbl[1024] u16: bit 15 clear: symbol | len << 8 (len <= 10); bit 15 set: continue
// the tree walk from internal node (entry & 0x1FF) after 10 bits; 0xFFFF: invalid.
// child[2 * 256] u16: < 256 leaf symbol, 256 + k internal node k.  A bad tree sets kDErrTree and
// lowers *badq (when given) to its stream.
__global__ __launch_bounds__(64) void k_dtable(const uint8_t *in, uint32_t nblocks, const DStream *ds,
                                               uint16_t *tbl, uint16_t *child, uint32_t *err, uint32_t *badq) {
    __shared__ uint16_t ch[512];
    __shared__ uint16_t par[256];    // parent node | side << 15; 0xFFFF = none
    __shared__ uint8_t dep[256];
    __shared__ uint32_t code[256];
    __shared__ uint32_t bad;
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    if (q >= 4 * nblocks) return;
    const DStream s = ds[q];
    if (s.raw || s.ts == 0 || s.count == 0) return;
    const uint32_t ts = s.ts, real = ts + 1;
    const uint64_t bm_off = s.pairs_off - (2 * ts + 7) / 8;
    if (lane == 0) bad = 0;
    for (uint32_t k = lane; k < 256; k += 64) par[k] = 0xFFFF;
    __syncthreads();
    // children (1042-1057: an internal child k is stored as (256 - real) + k)
    for (uint32_t x = lane; x < 2 * ts; x += 64) {
        const bool internal = (in[bm_off + (x >> 3)] >> (x & 7)) & 1;
        uint32_t v = in[s.pairs_off + x];
        if (internal) {
            const uint32_t k = v - (256 - real);
            // a child is created before its parent: k < x / 2 keeps the tree acyclic
            if (v < 256 - real || k >= x / 2) { bad = 1; v = 0; }
            else v = 256 + k;
        }
        ch[x] = (uint16_t)v;
    }
    __syncthreads();
    for (uint32_t x = lane; x < 2 * ts; x += 64)
        if (ch[x] >= 256) {
            const uint32_t k = ch[x] - 256;
            if (par[k] != 0xFFFF) bad = 1;   // two parents
            par[k] = (uint16_t)((x >> 1) | ((x & 1) << 15));
        }
    __syncthreads();
    // depth and code of every internal node by walking to the root (ts - 1)
    for (uint32_t k = lane; k < ts; k += 64) {
        // gathered leaf-up, the branch at depth i ends in bit i (root first, LSB-first)
        uint32_t d = 0, cd = 0, n = k;
        while (n != ts - 1) {
            const uint32_t pv = par[n];
            if (pv == 0xFFFF || d >= 31) { bad = 1; break; }
            cd = (cd << 1) | (pv >> 15);
            n = pv & 0x7FFF;
            d++;
        }
        dep[k] = (uint8_t)d;
        code[k] = cd;
    }
    __syncthreads();
    uint16_t *T = tbl + 1024ull * q;
    uint16_t *C = child + 512ull * q;
    for (uint32_t x = lane; x < 1024; x += 64) T[x] = 0xFFFF;
    for (uint32_t x = lane; x < 2 * ts; x += 64) C[x] = ch[x];
    __syncthreads();
    __threadfence_block();
    for (uint32_t x = lane; x < 2 * ts; x += 64) {
        const uint32_t node = x >> 1, side = x & 1;
        const uint32_t d = dep[node] + 1u;
        if (d > 32) { bad = 1; continue; }
        const uint32_t cd = code[node] | (side << dep[node]);
        if (ch[x] < 256) {
            if (d <= kDTblBits) {
                const uint16_t e = (uint16_t)(ch[x] | (d << 8));
                for (uint32_t sfx = 0; sfx < (1u << (kDTblBits - d)); sfx++) T[cd | (sfx << d)] = e;
            }
        } else if (d == kDTblBits) {
            T[cd] = (uint16_t)(0x8000u | (ch[x] - 256));
        }
    }
    __syncthreads();
    if (lane == 0 && bad) {
        atomicOr(err, kDErrTree);
        if (badq) atomicMin(badq, q);
    }
}

// ---------------------------------------------------------------------------
// one workgroup per sub-stream: Huffman symbols into the symbol scratch.  64 VGPRs (a few
// spilled) for two workgroups per CU: the serial code walks are latency-bound, and twice
// the waves took text's symbol streams from 15.1 to 9.9 ms per GiB
__global__ __launch_bounds__(kDSymThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_dsyms(const uint8_t *in, uint64_t in_len, uint32_t nblocks,
                                                        const DStream *ds, const uint16_t *tbl, const uint16_t *child,
                                                        uint8_t *sym, const uint32_t *err, uint64_t *stats) {
    __shared__ uint16_t T[1u << kDTblBits];
    __shared__ uint16_t C[512];
    __shared__ uint32_t st[kDSymThreads + 1];
    __shared__ uint32_t cnt[kDSymThreads / 64];
    __shared__ uint32_t flag[2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (q >= 4 * nblocks || (*err & (kDErrRecord | kDErrHeader | kDErrTree | kDErrScratch))) return;
    const DStream s = ds[q];
    uint8_t *dst = sym + s.dst;
    if (s.raw) {
        if (tid == 0 && s.count) dst[0] = (uint8_t)s.rawv;
        return;
    }
    uint32_t got = 0;
    if (s.ts != 0 && s.count != 0) {
        for (uint32_t x = tid; x < (1u << kDTblBits); x += kDSymThreads) T[x] = tbl[(1ull << kDTblBits) * q + x];
        for (uint32_t x = tid; x < 2 * s.ts; x += kDSymThreads) C[x] = child[512ull * q + x];
        __syncthreads();
        // every code 8 bits long (a complete depth-8 tree: the chars of random data): the
        // codes are the stream's bytes (the words start on a byte), so symbol i is T[byte i]
        // - a byte substitution, no segment agreement
        static_assert(kDSymThreads == (1u << kDTblBits), "one table entry per lane");
        const uint32_t e = T[tid];
        if (__syncthreads_and(!(e & 0x8000u) && ((e >> 8) & 0x1Fu) == 8u)) {
            got = min(s.count, s.nbits / 8);
            const uintptr_t a = (uintptr_t)(in + (s.words_bit >> 3)), aw = a & ~(uintptr_t)3;
            const uint32_t sh = (uint32_t)(a & 3);
            const uint32_t *w = (const uint32_t *)aw;
            const uint64_t vlim = (uint64_t)((uintptr_t)in + in_len - aw);   // valid bytes from w
            const uint64_t wlim = vlim / 4;                                   // whole dwords from w
            const uint32_t ndw = (got + 3) / 4;
            uint32_t *d32 = (uint32_t *)dst;
            // output dword j = lane + 1024 i: consecutive lanes touch consecutive dwords (loads
            // and stores coalesce); kU dwords per lane and step, all loads in flight together
            auto ld = [&](uint64_t wi) -> uint32_t {
                if (wi < wlim) return w[wi];
                uint32_t x = 0;   // the buffer's last partial dword, byte by byte
                for (uint32_t q = 0; q < 4; q++)
                    if (4 * wi + q < vlim) x |= (uint32_t)((const uint8_t *)aw)[4 * wi + q] << (8 * q);
                return x;
            };
            constexpr uint32_t kU = 4;
            for (uint32_t j00 = tid; j00 < ndw; j00 += kDSymThreads * kU) {
                uint32_t v0[kU], v1[kU];
#pragma unroll
                for (uint32_t u = 0; u < kU; u++) {
                    const uint32_t j = j00 + kDSymThreads * u;
                    v0[u] = j < ndw ? ld(j) : 0u;
                    v1[u] = j < ndw ? ld((uint64_t)j + 1) : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < kU; u++) {
                    const uint32_t j = j00 + kDSymThreads * u;
                    if (j >= ndw) break;
                    const uint32_t c = __builtin_amdgcn_alignbyte(v1[u], v0[u], sh);
                    uint32_t o = 0;
#pragma unroll
                    for (uint32_t q = 0; q < 4; q++)
                        if (4 * j + q < got) o |= (uint32_t)(T[(c >> (8 * q)) & 0xFFu] & 0xFFu) << (8 * q);
                    d32[j] = o;   // (bytes past `got` are zero, as the tail below writes them)
                }
            }
        } else {
            uint64_t bit0;
            const BitBuf src = make_bits(in, in_len, bit0);
            got = seg_decode<false>(src, bit0 + s.words_bit, s.nbits, s.count, T, C, dst, nullptr, st, cnt, flag, stats);
        }
    }
    // symbols the words do not cover stay zero (the reference memsets, 1107-1187)
    for (uint32_t x = got + tid; x < s.count; x += kDSymThreads) dst[x] = 0;
}

// one workgroup per block: the pCnt Golomb-Rice lengths from the decoded golomb bytes
__global__ __launch_bounds__(kDSymThreads) void k_dgolomb(uint32_t nblocks, DBlock *blk, const DStream *ds,
                                                          const uint8_t *sym, uint32_t *glen, uint32_t *err,
                                                          uint64_t *stats) {
    __shared__ uint32_t st[kDSymThreads + 1];
    __shared__ uint32_t cnt[kDSymThreads / 64];
    __shared__ uint32_t flag[2];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b >= nblocks || (*err & (kDErrRecord | kDErrHeader | kDErrTree | kDErrScratch))) return;
    DBlock &B = blk[b];
    const uint32_t pcnt = B.pcnt;
    uint32_t got = 0;
    if (pcnt > 0) {
        const DStream s = ds[4ull * b + 3];
        const uint64_t nbytes = 4ull * B.G;
        uint64_t bit0;
        const BitBuf src = make_bits(sym + s.dst, nbytes, bit0);
        got = seg_decode<true>(src, bit0, (uint32_t)(8 * nbytes), pcnt, nullptr, nullptr, nullptr,
                               glen + B.glen_off, st, cnt, flag, stats + kSsGolomb);
    }
    if (tid == 0) {
        B.glen_got = got;
        if (got < pcnt) atomicOr(err, kDErrGolomb);   // golomb stream too short: FORMAT
    }
}

// ---------------------------------------------------------------------------

// one workgroup per block: tokens decoded (the reference stops at the first match
// token past pCnt, 2331-2335), matches among them, decoded length
__global__ __launch_bounds__(256) void k_dlen(uint32_t nblocks, DBlock *blk, const uint8_t *sym,
                                              const uint32_t *glen, uint32_t *err) {
    __shared__ uint32_t sh[4];
    __shared__ uint64_t sh64[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b >= nblocks) return;
    DBlock &B = blk[b];
    if (*err & (kDErrRecord | kDErrHeader | kDErrTree | kDErrScratch | kDErrGolomb)) {
        if (tid == 0) B.out_len = 0;
        return;
    }
    const uint8_t *fl = sym + B.sym_off;
    const uint32_t N = B.N, pcnt = B.pcnt;
    uint32_t z = 0;
    for (uint32_t x = tid; x < B.nb; x += 256) {
        const uint32_t valid = min(8u, N - 8 * x);
        z += (uint32_t)__builtin_popcount(~(uint32_t)fl[x] & ((1u << valid) - 1u));
    }
    uint32_t Z;
    (void)block_xscan(z, sh, &Z);
    uint32_t n_eff = N, pc_eff = Z;
    if (Z > pcnt) {   // more match flags than distances: stop at the (pcnt+1)-th match token
        pc_eff = pcnt;
        if (tid == 0) {
            uint32_t seen = 0, t = 0;
            for (; t < N; t++)
                if (!((fl[t >> 3] >> (t & 7)) & 1)) {
                    if (seen == pcnt) break;
                    seen++;
                }
            sh[0] = t;
        }
        __syncthreads();
        n_eff = sh[0];
        __syncthreads();
    }
    // the reference encoder emits l in [3, 257] (1459-1462); a longer length is malformed
    // here (it could not fit an LZ step), the only stream the host decoder would take
    uint64_t s = 0;
    bool longl = false;
    for (uint32_t i = tid; i < pc_eff; i += 256) {
        const uint32_t l = glen[B.glen_off + i];
        longl = longl || l >= kMaxL;
        s += l;
    }
    if (longl) atomicOr(err, kDErrHeader);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) sh64[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const uint64_t tot = (uint64_t)n_eff + sh64[0] + sh64[1] + sh64[2] + sh64[3];
        B.n_eff = n_eff;
        B.pc_eff = pc_eff;
        if (tot > 0xFFFFFFFFull) { atomicOr(err, kDErrHeader); B.out_len = 0; }
        else B.out_len = (uint32_t)tot;
    }
}

// output offsets of the blocks; total into words[kDwTotal]; capacity check
__global__ void k_dscan_out(uint32_t nblocks, DBlock *blk, uint64_t cap, uint64_t *words, uint32_t *err) {
    __shared__ uint64_t sh[16];
    __shared__ uint64_t carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nblocks; b0 += blockDim.x) {
        const uint32_t b = b0 + tid;
        const uint64_t v = b < nblocks ? blk[b].out_len : 0;
        uint64_t inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t t = __shfl_up(inc, o, 64);
            if (lane >= (uint32_t)o) inc += t;
        }
        if (lane == 63) sh[wv] = inc;
        __syncthreads();
        uint64_t pre = carry + inc - v, all = 0;
        for (uint32_t w = 0; w < blockDim.x / 64; w++) {
            if (w < wv) pre += sh[w];
            all += sh[w];
        }
        if (b < nblocks) blk[b].out_off = pre;
        __syncthreads();
        if (tid == 0) carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        words[kDwTotal] = carry;
        if (carry > cap) atomicOr(err, kDErrOutCap);
    }
}

// one workgroup per block: tokens -> bytes (my_LZ77_decompress 1716-1735).  64 VGPRs and
// four tokens per lane (74 KB of LDS): two workgroups per CU hide the steps' barriers and
// loads (rand 5.3 -> 4.2 ms per GiB, text 8.2 -> 5.7)
constexpr uint32_t kRes = 0x80000000u;   // lk entry: resolved byte (low 8 bits), else link (LDS index)
constexpr uint32_t kHist = 2048;

__device__ inline uint32_t block_xmax(uint32_t v, uint32_t *sh) {   // exclusive running max over threads
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc = max(inc, t);
    }
    if (lane == 63) sh[wv] = inc;
    uint32_t ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0;
    __syncthreads();
    for (uint32_t w = 0; w < wv && w < nw; w++) ex = max(ex, sh[w]);
    __syncthreads();
    return ex;
}

// kClip (a range decode, k_dlz_clip): only the decoded bytes [w.lo, w.hi) of the run are stored, byte
// w.lo at out[0]; a block is still expanded from its first token (a link reaches back 2047 bytes),
// but its step loop ends at the first step boundary at or past w.hi, and a block outside the window
// is not expanded.  *stored counts the bytes stored.
template <bool kClip>
__device__ __forceinline__ void dlz_body(uint32_t nblocks, const DBlock *blk, const DStream *ds, const uint8_t *sym,
                                         const uint32_t *glen, uint8_t *out, uint32_t *err, DClip w,
                                         unsigned long long *stored) {
    __shared__ uint8_t ob[kHist + kDLzTile];              // [history | this step's bytes]
    __shared__ __attribute__((aligned(16))) uint32_t lk[kDLzTile];   // token marks, then links / bytes
    __shared__ uint2 tr[kDLzTPT * kDLzThreads];                 // this step's tokens: off | L << 13 | ism << 22 | ok << 23, P | c << 16
    __shared__ uint32_t sh[16];
    __shared__ uint32_t s_any[2];
    __shared__ uint32_t s_used;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b >= nblocks || *err) return;
    const DBlock B = blk[b];
    const uint8_t *fl = sym + B.sym_off;
    const uint8_t *ch = sym + ds[4ull * b + 1].dst;
    const uint8_t *pb = sym + ds[4ull * b + 2].dst;
    const uint32_t *gl = glen + B.glen_off;
    uint8_t *o = out + B.out_off;
    // kClip: block bytes [clo, chi) are in the window; byte x of them goes to out[ob0 + x]
    uint32_t clo = 0, chi = 0;
    int64_t ob0 = 0;
    if (kClip) {
        if (B.out_off >= w.hi || B.out_off + B.out_len <= w.lo) return;   // (the whole workgroup)
        clo = w.lo > B.out_off ? (uint32_t)(w.lo - B.out_off) : 0u;
        chi = (uint32_t)min((uint64_t)B.out_len, w.hi - B.out_off);
        ob0 = (int64_t)B.out_off - (int64_t)w.lo;
    }
    auto put = [&](uint32_t x, uint8_t v) {   // decoded byte x of the block
        if (!kClip) o[x] = v;
        else if (x >= clo && x < chi) out[ob0 + x] = v;
    };
    auto count = [&](uint32_t x0, uint32_t n) {   // kClip: bytes [x0, x0 + n) are done
        if (kClip && tid == 0) {
            const uint32_t a = max(x0, clo), e = min(x0 + n, chi);
            if (e > a) atomicAdd(stored, (unsigned long long)(e - a));
        }
    };
    const uint32_t n_eff = B.n_eff;
    uint32_t tc = 0, mc = 0, oc = 0;
    uint32_t window = kDLzTPT * kDLzThreads;   // tokens read per step, adapted to the token length seen
    bool bad = false;
    while (tc < n_eff) {
        if (kClip && oc >= chi) break;   // the window ends before this step
        const uint32_t limit = min(n_eff, tc + window);
        uint32_t len[kDLzTPT], L[kDLzTPT], P[kDLzTPT], c[kDLzTPT];
        bool ism[kDLzTPT], valid[kDLzTPT];
        uint32_t nm = 0;
#pragma unroll
        for (uint32_t u = 0; u < kDLzTPT; u++) {
            const uint32_t t = tc + kDLzTPT * tid + u;
            valid[u] = t < limit;
            ism[u] = valid[u] && !((fl[t >> 3] >> (t & 7)) & 1u);
            c[u] = valid[u] ? ch[t] : 0u;
            nm += ism[u] ? 1u : 0u;
        }
        uint32_t mtot;
        uint32_t rank = mc + block_xscan(nm, sh, &mtot);
        if (mtot == 0) {
            // literal tokens only (random data): the bytes are the chars, one per token
            const uint32_t cnt = limit - tc;
#pragma unroll
            for (uint32_t u = 0; u < kDLzTPT; u++)
                if (valid[u]) put(oc + kDLzTPT * tid + u, (uint8_t)c[u]);
            count(oc, cnt);
            // history = the last 2 KiB of [history | these bytes]
            uint8_t h[kHist / kDLzThreads];
#pragma unroll
            for (uint32_t q = 0; q < kHist / kDLzThreads; q++) {
                const uint32_t j = cnt + tid + q * kDLzThreads;   // index in [history | bytes]
                h[q] = j < kHist ? ob[j] : ch[tc + j - kHist];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t q = 0; q < kHist / kDLzThreads; q++) ob[tid + q * kDLzThreads] = h[q];
            __syncthreads();
            oc += cnt;
            tc += cnt;
            window = kDLzTPT * kDLzThreads;
            continue;
        }
        uint32_t lsum = 0;
#pragma unroll
        for (uint32_t u = 0; u < kDLzTPT; u++) {
            L[u] = 0; P[u] = 0;
            if (ism[u]) {
                L[u] = gl[rank];
                const uint32_t bit = kPBits * rank, k = bit >> 3;
                P[u] = ((pb[k] | (pb[k + 1] << 8) | (pb[k + 2] << 16)) >> (bit & 7)) & 0x7FFu;   // decombine_bits
                rank++;
            }
            len[u] = valid[u] ? (ism[u] ? L[u] + 1 : 1u) : 0u;
            lsum += len[u];
        }
        uint32_t ltot;
        uint32_t off = block_xscan(lsum, sh, &ltot);
        // clear the token marks of this step's tile (8 slots per lane, two 16-B stores)
        ((uint4 *)lk)[2 * tid] = make_uint4(0, 0, 0, 0);
        ((uint4 *)lk)[2 * tid + 1] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        // the tokens whose output fits the tile (a prefix): record + mark at their first byte
        uint32_t taken = 0, mtaken = 0, end = 0;
#pragma unroll
        for (uint32_t u = 0; u < kDLzTPT; u++) {
            if (valid[u] && off + len[u] <= kDLzTile) {
                taken++;
                // a distance before the block start is malformed (reference: Fatal Error,
                // :1727); its bytes resolve to 0 and the error is reported
                const bool okp = !ism[u] || (P[u] != 0 && P[u] <= oc + off);
                bad = bad || !okp;
                mtaken += ism[u] ? 1u : 0u;
                tr[kDLzTPT * tid + u] = make_uint2(off | (L[u] << 13) | ((ism[u] ? 1u : 0u) << 22) | ((okp ? 1u : 0u) << 23),
                                             P[u] | (c[u] << 16));
                lk[off] = kDLzTPT * tid + u + 1;
                end = off + len[u];
            }
            off += len[u];
        }
        uint32_t ttot, mt2;
        (void)block_xscan(taken, sh, &ttot);
        (void)block_xscan(mtaken, sh, &mt2);
        uint32_t umax = end;
        for (int o2 = 32; o2 > 0; o2 >>= 1) umax = max(umax, __shfl_xor(umax, o2, 64));
        if (tid == 0) s_used = 0;
        __syncthreads();
        if ((tid & 63) == 0) atomicMax(&s_used, umax);
        // every position finds its token: running max of the marks over positions
        const uint4 m0 = ((const uint4 *)lk)[2 * tid], m1 = ((const uint4 *)lk)[2 * tid + 1];
        uint32_t mk[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
        uint32_t run = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) { run = max(run, mk[j]); mk[j] = run; }
        const uint32_t carry = block_xmax(run, sh);
        const uint32_t used = s_used;
        uint32_t val[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t x = 8 * tid + j;
            val[j] = 0;
            if (x < used) {
                const uint2 r = tr[max(carry, mk[j]) - 1];
                const uint32_t toff = r.x & 0x1FFFu, tl = (r.x >> 13) & 0x1FFu;
                const uint32_t k = x - toff;
                if (!((r.x >> 22) & 1u) || k == tl) val[j] = kRes | (r.y >> 16);
                else if (!((r.x >> 23) & 1u)) val[j] = kRes;
                else {
                    const uint32_t li = kHist + x - (r.y & 0xFFFFu);
                    val[j] = li < kHist ? (kRes | ob[li]) : li;
                }
            }
        }
        __syncthreads();   // all marks read before the links replace them
        ((uint4 *)lk)[2 * tid] = make_uint4(val[0], val[1], val[2], val[3]);
        ((uint4 *)lk)[2 * tid + 1] = make_uint4(val[4], val[5], val[6], val[7]);
        __syncthreads();
        // pointer jumping: lk[x] <- lk[lk[x]] until every byte is resolved (links point back)
        for (uint32_t r = 0;; r++) {
            if (tid == 0) s_any[r & 1] = 0;
            __syncthreads();
            bool any = false;
            for (uint32_t x = tid; x < used; x += kDLzThreads) {
                const uint32_t v = lk[x];
                if (!(v & kRes)) {
                    const uint32_t w = v < kHist ? (kRes | ob[v]) : lk[v - kHist];
                    lk[x] = w;
                    any = any || !(w & kRes);
                }
            }
            if (any) s_any[r & 1] = 1;
            __syncthreads();
            if (!s_any[r & 1]) break;
        }
        for (uint32_t x = tid; x < used; x += kDLzThreads) {
            const uint8_t v = (uint8_t)lk[x];
            ob[kHist + x] = v;
            put(oc + x, v);
        }
        count(oc, used);
        __syncthreads();
        // history = the last 2 KiB of [history | step bytes]
        const uint8_t h0 = ob[used + tid], h1 = ob[used + tid + kDLzThreads];
        __syncthreads();
        ob[tid] = h0;
        ob[tid + kDLzThreads] = h1;
        __syncthreads();
        oc += used;
        tc += ttot;
        mc += mt2;
        if (ttot == 0) { bad = true; break; }   // cannot happen for l <= 257 (k_dlen)
        // next window: enough tokens for about 1.25 tiles at this step's mean length
        window = min(kDLzTPT * kDLzThreads, max(256u, (uint32_t)(5ull * kDLzTile * ttot / (4ull * max(used, 1u)))));
    }
    if (bad) atomicOr(err, kDErrDist);
}

__global__ __launch_bounds__(kDLzThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_dlz(uint32_t nblocks, const DBlock *blk, const DStream *ds,
                                                     const uint8_t *sym, const uint32_t *glen, uint8_t *out,
                                                     uint32_t *err) {
    dlz_body<false>(nblocks, blk, ds, sym, glen, out, err, DClip{}, nullptr);
}

__global__ __launch_bounds__(kDLzThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_dlz_clip(uint32_t nblocks, const DBlock *blk, const DStream *ds,
                                                          const uint8_t *sym, const uint32_t *glen, uint8_t *out,
                                                          uint32_t *err, DClip w, unsigned long long *stored) {
    dlz_body<true>(nblocks, blk, ds, sym, glen, out, err, w, stored);
}

// ---- the size pass and the range decode (fcx_range.hip) ----
// the size pass's list of sub-streams to decode: sel[2b] = block b's flags, sel[2b + 1] = its Golomb
// bytes, the rest of the nsel entries (a multiple of 4, as k_dtable and k_dsyms count) empty
__global__ void k_dsel(uint32_t nblocks, uint32_t nsel, const DStream *ds, DStream *sel) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nsel) return;
    DStream s{};
    s.raw = 1;
    if (x < 2 * nblocks) s = ds[4ull * (x >> 1) + 3 * (x & 1)];
    sel[x] = s;
}

// thread per block: the size pass's results as plain arrays (payload offset and length, decoded size)
__global__ void k_dsizes_out(uint32_t nblocks, const DBlock *blk, uint64_t *roff, uint32_t *rlen, uint32_t *dsize) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    roff[b] = blk[b].payload_off;
    rlen[b] = blk[b].payload_len;
    dsize[b] = blk[b].out_len;
}

// thread per block of a sub-run: its decoded size against the index's (dec_off: the sub-run's first entry)
__global__ void k_dcheck_sizes(uint32_t nblocks, const DBlock *blk, const uint64_t *dec_off, uint32_t *err) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks || *err) return;
    if (dec_off[b + 1] - dec_off[b] != (uint64_t)blk[b].out_len) atomicOr(err, kDErrIndex);
}

// the full decode's stages behind the header pass (dec7_heads)
void dec_launch(const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out, uint64_t cap, DBlock *blk,
                DStream *ds, uint16_t *tbl, uint16_t *child, uint8_t *sym, uint32_t *glen, uint64_t *words,
                uint32_t *err, hipStream_t st, hipEvent_t *ev) {
    auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i], st); };
    mark(0);
    hipLaunchKernelGGL(k_dtable, dim3(4 * nblocks), dim3(64), 0, st, d_in, nblocks, ds, tbl, child, err, (uint32_t *)nullptr);
    mark(1);
    hipLaunchKernelGGL(k_dsyms, dim3(4 * nblocks), dim3(kDSymThreads), 0, st, d_in, in_len, nblocks, ds, tbl, child, sym, err,
                       words + kDwStats);
    mark(2);
    hipLaunchKernelGGL(k_dgolomb, dim3(nblocks), dim3(kDSymThreads), 0, st, nblocks, blk, ds, sym, glen, err, words + kDwStats);
    mark(3);
    hipLaunchKernelGGL(k_dlen, dim3(nblocks), dim3(256), 0, st, nblocks, blk, sym, glen, err);
    hipLaunchKernelGGL(k_dscan_out, dim3(1), dim3(1024), 0, st, nblocks, blk, cap, words, err);
    mark(4);
    hipLaunchKernelGGL(k_dlz, dim3(nblocks), dim3(kDLzThreads), 0, st, nblocks, blk, ds, sym, glen, d_out, err);
    mark(5);
}

void dec_launch_tables8(const uint8_t *d_in, uint32_t nstreams, const DStream *ds, uint16_t *tbl, uint16_t *child,
                        uint32_t *err, uint32_t *badq, hipStream_t st) {
    hipLaunchKernelGGL(k_dtable, dim3(nstreams), dim3(64), 0, st, d_in, nstreams / 4, ds, tbl, child, err, badq);
}

void dec_launch_syms8(const uint8_t *d_in, uint64_t in_len, uint32_t nstreams, const DStream *ds,
                      const uint16_t *tbl, const uint16_t *child, uint8_t *sym, const uint32_t *err,
                      uint64_t *stats, hipStream_t st) {
    hipLaunchKernelGGL(k_dsyms, dim3(nstreams), dim3(kDSymThreads), 0, st, d_in, in_len, nstreams / 4, ds, tbl, child, sym,
                       err, stats);
}

// The scratch per block of a call, the record walk, the header pass and the scratch offsets of the
// sub-streams of smask; waits for the stream to size the symbol scratch from the totals.
static int dec7_heads(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint32_t smask, hipStream_t st) {
    Dec7 &D = c->d7;
    if (nblocks > D.cap_blocks) {
        static_cast<Dec7Blocks &>(D) = Dec7Blocks{};   // (the old scratch goes before the new is made)
        FCX_TRY(D.blk.reserve(sizeof(DBlock) * (uint64_t)nblocks, "blocks"));
        FCX_TRY(D.ds.reserve(sizeof(DStream) * 4ull * nblocks, "streams"));
        FCX_TRY(D.ds_sel.reserve(sizeof(DStream) * (2ull * nblocks + 4), "size pass streams"));
        FCX_TRY(D.symb.reserve(8ull * nblocks, "symb"));
        FCX_TRY(D.tbl.reserve(2048ull * 4 * nblocks, "tables"));
        FCX_TRY(D.child.reserve(1024ull * 4 * nblocks, "children"));
        D.cap_blocks = nblocks;
    }
    uint64_t *hw = D.host_words;
    uint32_t *err = (uint32_t *)(D.words + kDwErr);
    memset(hw + kDwStats, 0, kSsWords * sizeof(uint64_t));
    FCX_HIP(hipMemsetAsync(D.words, 0, 8 * kDwWords, st));
    hipLaunchKernelGGL(k_dindex, dim3(1), dim3(1), 0, st, d_in, in_len, nblocks, D.blk, err);
    hipLaunchKernelGGL(k_dhead, dim3((nblocks + 255) / 256), dim3(256), 0, st, d_in, nblocks, D.blk, D.ds, D.symb, smask, err);
    hipLaunchKernelGGL(k_dscan, dim3(1), dim3(1024), 0, st, nblocks, D.blk, D.ds, D.symb, smask, D.words + kDwSymBytes);
    FCX_HIP(hipMemcpyAsync(hw, D.words, 8 * (kDwGolombVals + 1), hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    if ((uint32_t)hw[kDwErr] & (kDErrRecord | kDErrHeader)) return fail(FCX_ERR_FORMAT, "malformed block records / headers");
    FCX_TRY(D.sym.reserve(hw[kDwSymBytes] + 64, "symbols"));
    FCX_TRY(D.glen.reserve(4 * hw[kDwGolombVals] + 64, "golomb values"));
    return FCX_OK;
}

// the stages every pass runs on the sub-streams of smask, up to the decoded sizes (k_dlen)
static void dec7_launch_sizes(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint32_t smask,
                              hipStream_t st) {
    Dec7 &D = c->d7;
    uint32_t *err = (uint32_t *)(D.words + kDwErr);
    // tables and symbols of the sub-streams of smask: of all four in place, or of the flags and the
    // Golomb bytes through a list of just those descriptors (k_dsel), the way the FCX8 decoder hands
    // its char streams to the same two kernels
    const DStream *ds = D.ds;
    uint32_t nstreams = 4 * nblocks;
    if (smask != kAllStreams) {
        nstreams = (2 * nblocks + 3) & ~3u;
        hipLaunchKernelGGL(k_dsel, dim3((nstreams + 255) / 256), dim3(256), 0, st, nblocks, nstreams, D.ds, D.ds_sel);
        ds = D.ds_sel;
    }
    hipLaunchKernelGGL(k_dtable, dim3(nstreams), dim3(64), 0, st, d_in, nstreams / 4, ds, D.tbl, D.child, err,
                       (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_dsyms, dim3(nstreams), dim3(kDSymThreads), 0, st, d_in, in_len, nstreams / 4, ds, D.tbl, D.child,
                       D.sym, err, D.words + kDwStats);
    hipLaunchKernelGGL(k_dgolomb, dim3(nblocks), dim3(kDSymThreads), 0, st, nblocks, D.blk, D.ds, D.sym, D.glen, err,
                       D.words + kDwStats);
    hipLaunchKernelGGL(k_dlen, dim3(nblocks), dim3(256), 0, st, nblocks, D.blk, D.sym, D.glen, err);
}

static int dec7_verdict(fcx_dctx *c, hipStream_t st) {
    Dec7 &D = c->d7;
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(D.host_words, D.words, 8 * kDwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    const uint32_t e = (uint32_t)D.host_words[kDwErr];
    if (e & kDErrIndex) return fail(FCX_ERR_FORMAT, "the index disagrees with the run: a touched record's decoded size differs");
    if (e) return fail(FCX_ERR_FORMAT, "malformed stream (decoder error bits " + std::to_string(e) + ")");
    return FCX_OK;
}

int dec7_sizes(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint64_t *d_roff, uint32_t *d_rlen,
               uint32_t *d_dsize, hipStream_t st) {
    FCX_TRY(dec7_heads(c, d_in, in_len, nblocks, kSizeStreams, st));
    dec7_launch_sizes(c, d_in, in_len, nblocks, kSizeStreams, st);
    hipLaunchKernelGGL(k_dsizes_out, dim3((nblocks + 255) / 256), dim3(256), 0, st, nblocks, c->d7.blk, d_roff, d_rlen, d_dsize);
    return dec7_verdict(c, st);
}

int dec7_range(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, const uint64_t *d_dec_off, DClip w,
               uint8_t *d_out, hipStream_t st, uint64_t *stored) {
    Dec7 &D = c->d7;
    FCX_TRY(dec7_heads(c, d_in, in_len, nblocks, kAllStreams, st));
    dec7_launch_sizes(c, d_in, in_len, nblocks, kAllStreams, st);
    uint32_t *err = (uint32_t *)(D.words + kDwErr);
    hipLaunchKernelGGL(k_dscan_out, dim3(1), dim3(1024), 0, st, nblocks, D.blk, ~0ull, D.words, err);
    hipLaunchKernelGGL(k_dcheck_sizes, dim3((nblocks + 255) / 256), dim3(256), 0, st, nblocks, D.blk, d_dec_off, err);
    hipLaunchKernelGGL(k_dlz_clip, dim3(nblocks), dim3(kDLzThreads), 0, st, nblocks, D.blk, D.ds, D.sym, D.glen, d_out, err, w,
                       (unsigned long long *)(D.words + kDwStored));
    FCX_TRY(dec7_verdict(c, st));
    *stored = D.host_words[kDwStored];
    return FCX_OK;
}

}  // namespace fcx

// ---------------------------------------------------------------------------
// C ABI (include/fcx.h): decoder context, device and host entry points
using namespace fcx;

namespace {
const char *kDStageNames[] = {"tables", "symbols", "golomb", "lengths", "lz"};
static_assert(sizeof(kDStageNames) / sizeof(kDStageNames[0]) == kDStages, "FCX7 stage names");
}  // namespace

extern "C" {

int fcx_dctx_create(fcx_dctx **out, int device) {
    if (!out) return fail(FCX_ERR_ARG, "fcx_dctx_create: NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FCX_ERR_HIP, "no HIP device: the GPU decoder needs one");
    if (device < 0 || device >= ndev) return fail(FCX_ERR_ARG, "bad device index");
    FCX_HIP(hipSetDevice(device));
    std::unique_ptr<fcx_dctx, Calls<fcx_dctx_destroy>> c(new fcx_dctx());
    c->device = device;
    if (c->d7.host_words.alloc(8 * kDwWords) != hipSuccess || c->d7.words.alloc(8 * kDwWords) != hipSuccess)
        return fail(FCX_ERR_NOMEM, "fcx_dctx_create: allocation failed");
    *out = c.release();
    return FCX_OK;
}

void fcx_dctx_destroy(fcx_dctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
}

int fcx_dctx_set_profiling(fcx_dctx *c, int enable) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    c->profiling = enable != 0;
    return FCX_OK;
}

int fcx_dctx_stage_count(fcx_dctx *c) { return c ? c->times.n : 0; }

int fcx_dctx_stage(fcx_dctx *c, int i, const char **name, float *ms) {
    if (!c || i < 0 || i >= c->times.n)   // (only an FCX8 call's table rules out "not profiled")
        return fail(FCX_ERR_ARG, c && c->times.n == kD78Stages ? "bad stage" : "bad stage / not profiled");
    return c->times.stage(i, name, ms);
}

int fcx_decompress_shard(fcx_dctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t nblocks, uint8_t *d_out,
                         uint64_t cap, uint64_t *out_len, void *stream) {
    if (!c || (in_len && !d_in) || (cap && !d_out)) return fail(FCX_ERR_ARG, "fcx_decompress_shard: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    FCX_HIP(hipSetDevice(c->device));
    c->times.reset();
    if (nblocks == 0) {
        if (out_len) *out_len = 0;
        return FCX_OK;
    }
    Dec7 &D = c->d7;
    FCX_TRY(dec7_heads(c, d_in, in_len, nblocks, kAllStreams, st));
    uint64_t *hw = D.host_words;
    uint32_t *err = (uint32_t *)(D.words + kDwErr);
    if (c->profiling) c->times.publish(kDStageNames, kDStages, true);
    dec_launch(d_in, in_len, nblocks, d_out, cap, D.blk, D.ds, D.tbl, D.child, D.sym, D.glen, D.words, err, st,
               c->profiling ? c->times.events() : nullptr);
    FCX_HIP(hipGetLastError());
    FCX_HIP(hipMemcpyAsync(hw, D.words, 8 * kDwWords, hipMemcpyDeviceToHost, st));
    FCX_HIP(hipStreamSynchronize(st));
    static const bool dbg = getenv("FCX_DEC_DEBUG") != nullptr;
    if (dbg) {
        const uint64_t *s = hw + kDwStats;
        fprintf(stderr, "fcx decode: symbol streams rounds %llu fallbacks %llu (flags %llu chars %llu p %llu golomb %llu)"
                " | golomb rounds %llu fallbacks %llu\n",
                (unsigned long long)s[kSsRounds], (unsigned long long)s[kSsFallbacks],
                (unsigned long long)s[kSsKind], (unsigned long long)s[kSsKind + 1],
                (unsigned long long)s[kSsKind + 2], (unsigned long long)s[kSsKind + 3],
                (unsigned long long)s[kSsGolomb + kSsRounds], (unsigned long long)s[kSsGolomb + kSsFallbacks]);
    }
    const uint32_t e = (uint32_t)hw[kDwErr];
    if (e & kDErrOutCap) return fail(FCX_ERR_CAPACITY, "output capacity too small");
    if (e) return fail(FCX_ERR_FORMAT, "malformed stream (decoder error bits " + std::to_string(e) + ")");
    if (out_len) *out_len = hw[kDwTotal];
    return FCX_OK;
}

int fcx_dctx_symbol_stats(fcx_dctx *c, uint64_t *out, int n) {
    if (!c || !out || n < 0) return fail(FCX_ERR_ARG, "fcx_dctx_symbol_stats: bad argument");
    // the statistics block as the last fcx_decompress_shard call read it back, in the order of fcx.h
    static const uint32_t kWord[FCX_DSYMBOL_STATS] = {kSsRounds, kSsFallbacks, kSsKind, kSsKind + 1, kSsKind + 2, kSsKind + 3,
                                                      kSsGolomb + kSsRounds, kSsGolomb + kSsFallbacks};
    for (int i = 0; i < n && i < FCX_DSYMBOL_STATS; i++) out[i] = c->d7.host_words[kDwStats + kWord[i]];
    return FCX_OK;
}

int fcx_dctx_device(fcx_dctx *c, int *device) {
    if (!c) return fail(FCX_ERR_ARG, "NULL ctx");
    if (device) *device = c->device;
    return FCX_OK;
}

}  // extern "C"

