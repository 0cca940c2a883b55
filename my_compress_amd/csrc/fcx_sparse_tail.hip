// fcx_sparse_tail.hip — the sparse unit's second phase: one wave per listed tile (gfx950).
//
// k_match_sparse ends a few-match tile after its equal-key search (sparse_pairs, fcx_match.hip): what is
// left -- a handful of queries against a handful of candidates, then the parse of at most 64 matches
// -- is serial, latency-bound work for one wave, and an eight-wave workgroup holding a quarter of a
// CU's LDS and wave slots only waits through it.  Here a wave takes a listed tile:
// it stages the tile's window [t0 - 2048, t1 + 260) into its own LDS slice (16-byte loads, all in
// flight), reads R from the tile's mtok slot, runs the queries through scan_candidate -- the
// workgroup's own device code on the same byte image, so the same matches -- and publishes what the
// workgroup's queries and sparse_parse publish: m rows at the match positions, the tile's mbits
// words, chain words, prefix words, tinfo and the compact match list (over R in the mtok slot).
// No query comes out unknown: phase 1 keeps a tile whose R entry has more candidates than the
// extension budget.
//
// k_match_sparse marks a listed tile by a plain store to its tail flag (a shared list counter there
// cost a returning atomic on one address at the end of 4 tiles in 10); k_sparse_tail_list gathers
// the flagged tiles into a list with one atomic per 1024 tiles.  The tail kernel's grid is fixed and
// every wave strides over the list by the length read on the device: no host read-back, no grid
// from an estimate.
#define FCX_SPARSE 1
#define FCX_UNIT_NAME sparse
#define FCX_TAIL 1
#include "fcx_match.hip"   // scan_candidate and the helpers, under the sparse unit's switches

namespace fcx {

// sparse_parse (fcx_match.hip) with the ordered matches in lane registers: lane i < nm holds the i-th
// match position of the tile (pos, tile-relative), its length Lv and its m (resv).  Publishes the
// same chain words, prefix words, compact match list and tile totals.
__device__ inline void sparse_parse_lanes(uint32_t pos, uint32_t Lv, uint32_t resv, uint32_t nm, uint32_t nt, uint32_t t0,
                                          uint64_t *cw, uint64_t *pfx, uint32_t *ti, uint32_t *mt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwords = (nt + 63) / 64;
    // the chain takes a match when it reaches it (uniform walk over the ordered list)
    uint64_t tk = 0;
    uint32_t cur = 0;
    for (uint32_t i = 0; i < nm; i++) {
        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)i);
        if (p >= cur) {
            tk |= 1ull << i;
            cur = p + (uint32_t)__builtin_amdgcn_readlane((int)Lv, (int)i) + 1;
        }
    }
    // lane w: chain word w (literal tokens minus the taken matches' covered positions) and the
    // counts of the chain positions before it
    const uint32_t lo = 64 * lane;
    uint64_t cov = 0;
    uint32_t cov_before = 0, cov_tile = 0, mat_before = 0, gb_before = 0, gb_all = 0;
    for (uint64_t bits = tk; bits; bits &= bits - 1) {
        const uint32_t i = (uint32_t)__builtin_ctzll(bits);
        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)i);
        const uint32_t Lm = (uint32_t)__builtin_amdgcn_readlane((int)Lv, (int)i);
        const uint32_t c0 = p + 1, c1 = p + Lm + 1;   // covered positions [c0, c1)
        const uint32_t a = max(c0, lo), z = min(c1, lo + 64);
        if (a < z) cov |= (z - a == 64 ? ~0ull : ((1ull << (z - a)) - 1ull)) << (a - lo);
        cov_before += c1 <= lo ? c1 - c0 : (c0 < lo ? lo - c0 : 0u);
        cov_tile += min(c1, nt) - c0;
        const uint32_t g = (Lm >> 2) + 3;
        if (p < lo) { mat_before++; gb_before += g; }
        gb_all += g;
    }
    const uint32_t ntk = (uint32_t)__popcll(tk);
    if (lane < nwords) {
        const uint32_t nb = min(64u, nt - lo);
        const uint64_t valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
        cw[lane] = valid & ~cov;
        pfx[lane] = (uint64_t)(lo - cov_before) | ((uint64_t)mat_before << 13) | ((uint64_t)gb_before << 24);
    }
    if (lane < nm && ((tk >> lane) & 1ull)) mt[__popcll(tk & ((1ull << lane) - 1ull))] = resv;
    if (lane == 0) {
        ti[0] = 0u;
        ti[1] = t0 + max(cur, nt);
        ti[2] = nt - cov_tile;
        ti[3] = ntk;
        ti[4] = gb_all;
    }
}

constexpr uint32_t kImgVec = (kTileBytes / 4 + 4) / 4;   // 16-byte words of a window's byte image

__global__ __launch_bounds__(64) void k_sparse_tail(const uint8_t *__restrict__ in, Layout L, uint32_t *__restrict__ m,
                                                    uint64_t *__restrict__ mbits, uint64_t *__restrict__ chain,
                                                    uint64_t *__restrict__ chain_pfx, uint32_t *__restrict__ tinfo,
                                                    uint32_t *mtok) {
    __shared__ __attribute__((aligned(16))) uint32_t sdw[kTileBytes / 4 + 4];   // byte image of the window
    __shared__ uint32_t s_ord[3][64];   // the matches in position order: position, length, m
    const uint32_t lane = threadIdx.x;
    const uint32_t ntg = L.nblocks * L.tpb;
    const uint32_t *list = sparse_tail_list(mtok, ntg);
    const uint8_t *flags = sparse_tail_flags(mtok, ntg);
    const uint32_t cnt = min(uni(*sparse_tail_head(mtok, ntg)), ntg);   // (a tile is listed once at most)
    for (uint32_t p = blockIdx.x; p < cnt; p += gridDim.x) {
        const uint32_t bx = uni(list[p]);
        if (bx >= ntg) continue;
        // the tile's geometry, as match_tile has it
        const uint32_t b = bx / L.tpb, k = bx % L.tpb;
        const uint64_t bstart = (uint64_t)b * L.B;
        const uint32_t blen = (uint32_t)min((uint64_t)L.B, L.n - bstart);
        const uint32_t t0 = k * kTile;
        if (t0 >= blen) continue;
        const uint32_t t1 = min(blen, t0 + kTile);
        const uint32_t w0 = t0 >= 2048 ? t0 - 2048 : 0;
        const uint32_t nload = min(blen, t1 + kLookAhead) - w0;
        const uint32_t npos = t1 - w0, q0 = t0 - w0;
        uint32_t *mslot = mtok + (uint64_t)bx * kTileMatches;
        const uint32_t nr = min(uni((uint32_t)flags[bx]), kTailR);
        const uint32_t me = lane < nr ? mslot[lane] : 0u;   // R entry `lane`: position | key bits << 13
        // ---- stage bytes (zero padded), as match_tile does ----
        const uint8_t *src = in + bstart + w0;
        if ((((uintptr_t)src) & 15) == 0) {
            // the whole 16-byte words, all loads in flight; then the bytes of the one the block's end
            // cuts (LDS operations of a wave complete in order)
            uint4 v[(kImgVec + 63) / 64];
#pragma unroll
            for (uint32_t r = 0; r < (kImgVec + 63) / 64; r++) {
                const uint32_t v16 = lane + 64 * r;
                v[r] = make_uint4(0u, 0u, 0u, 0u);
                if (v16 < kImgVec && 16 * v16 + 16 <= nload) v[r] = ((const uint4 *)src)[v16];
            }
            const uint32_t cut = nload & ~15u;
            const uint32_t cb = cut + lane < nload ? (uint32_t)src[cut + lane] : 0u;
#pragma unroll
            for (uint32_t r = 0; r < (kImgVec + 63) / 64; r++)
                if (lane + 64 * r < kImgVec) ((uint4 *)sdw)[lane + 64 * r] = v[r];
            if (cut + lane < nload) ((uint8_t *)sdw)[cut + lane] = (uint8_t)cb;
        } else {
            for (uint32_t x = lane; x < kTileBytes / 4 + 4; x += 64) {
                uint32_t v = 0;
                for (uint32_t q = 0; q < 4; q++)
                    if (4 * x + q < nload) v |= (uint32_t)src[4 * x + q] << (8 * q);
                sdw[x] = v;
            }
        }
        __syncthreads();   // (one wave: orders the image's stores before the reads below)
        // ---- the queries: R entry `lane` against the R entries of its key bits in [x - 2047, x) ----
        const uint32_t x = me & 0x1FFFu;
        const uint32_t i = w0 + x;
        const bool q = lane < nr && !(x < q0 || x >= npos || i == 0 || blen - i < 4);
        const uint32_t cap = q ? min(kMaxL, blen - i) - 1 : 0u;
        const uint32_t xq = q ? x : 0u;
        const uint32_t qa = lds_ld4(sdw, xq), qb = lds_ld4(sdw, xq + 4), qc = lds_ld4(sdw, xq + 8);
        const uint32_t xlo = max(i, kWin) - kWin - w0;
        uint32_t best = 0, next = 0;
        bool unk = false;   // (stays false: at most kExtBudget candidates per entry, sparse_pairs)
        for (uint32_t e = 0; e < nr; e++) {
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)me, (int)e), xe = o & 0x1FFFu;
            if (q && !unk && ((o ^ me) >> 13) == 0 && xe < x && xe >= xlo)
                scan_candidate(sdw, xe, x, qa, qb, qc, cap, best, next, unk, 0u);
        }
        const uint32_t Lb = best >> 13, rel = x - q0;
        const bool hit = q && Lb >= kMinL;
        const uint32_t res = m_pack(Lb, x - (8191u - (best & 0x1FFFu)));
        if (hit) m[bstart + w0 + x] = res;
        // mbits word `lane` of the tile, and each match's rank in position order
        const uint64_t hm = __ballot(hit);
        uint64_t wm = 0;
        uint32_t rank = 0;
        for (uint64_t bits = hm; bits; bits &= bits - 1) {
            const uint32_t pr = (uint32_t)__builtin_amdgcn_readlane((int)rel, (int)__builtin_ctzll(bits));
            if ((pr >> 6) == lane) wm |= 1ull << (pr & 63);
            rank += pr < rel ? 1u : 0u;
        }
        const uint32_t nt = t1 - t0;
        if (lane < (nt + 63) / 64) mbits[(uint64_t)b * L.wpb + (t0 >> 6) + lane] = wm;
        if (hit) { s_ord[0][rank] = rel; s_ord[1][rank] = Lb; s_ord[2][rank] = res; }
        __syncthreads();
        const uint32_t nm = (uint32_t)__popcll(hm);
        const uint32_t pos = lane < nm ? s_ord[0][lane] : 0u, Lv = lane < nm ? s_ord[1][lane] : 0u,
                       resv = lane < nm ? s_ord[2][lane] : 0u;
        sparse_parse_lanes(pos, Lv, resv, nm, nt, t0, chain + (uint64_t)b * L.wpb + (uint64_t)k * (kTile / 64),
                           chain_pfx + (uint64_t)bx * (kTile / 64), tinfo + 8ull * bx, mslot);
        __syncthreads();   // the next tile's image and order overwrite the LDS this one read
    }
}

// The flagged tiles' indices into the list, in tile order within a workgroup's 1024 tiles: ranks by
// ballot, one reservation per workgroup.
constexpr uint32_t kTailListLanes = 1024;
__global__ __launch_bounds__(kTailListLanes) void k_sparse_tail_list(Layout L, uint32_t *mtok) {
    __shared__ uint32_t s_wsum[kTailListLanes / 64];
    __shared__ uint32_t s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t ntg = L.nblocks * L.tpb, bx = blockIdx.x * kTailListLanes + tid;
    const bool on = bx < ntg && sparse_tail_flags(mtok, ntg)[bx] != 0;
    const uint64_t bal = __ballot(on);
    if (lane == 0) s_wsum[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < kTailListLanes / 64; w++) tot += s_wsum[w];
        s_base = tot ? atomicAdd(sparse_tail_head(mtok, ntg), tot) : 0u;
    }
    __syncthreads();
    if (on) {
        uint32_t pos = s_base + lanes_below(bal);
        for (uint32_t w = 0; w < wv; w++) pos += s_wsum[w];
        if (pos < ntg) sparse_tail_list(mtok, ntg)[pos] = bx;
    }
}

void launch_sparse_tail(const MatchArgs &a, hipStream_t st) {
    const uint32_t ntg = a.L.nblocks * a.L.tpb;
    hipLaunchKernelGGL(k_sparse_tail_list, dim3((ntg + kTailListLanes - 1) / kTailListLanes), dim3(kTailListLanes), 0, st,
                       a.L, a.mtok);
    hipLaunchKernelGGL(k_sparse_tail, dim3(kTailGrid), dim3(64), 0, st, a.in, a.L, a.m, a.mbits, a.chain, a.chain_pfx,
                       a.tinfo, a.mtok);
}

}  // namespace fcx
