// fcx_sparse_tail.h — the sparse unit's two phases (fcx_match.hip under FCX_SPARSE, fcx_sparse_tail.hip;
// DESIGN.md §4c).  k_match_sparse ends a tile after the equal-key search: a tile without a candidate
// pair is all literals, written out before the filter; a tile with some (and at most kTailR entries in R) leaves
// R in its own mtok slot and R's length in its tail flag; k_sparse_tail_list gathers the flagged tiles
// into a list, and k_sparse_tail finishes each with one wave.
// Included by the sparse unit's translation units and the host layer only: the other match units'
// source does not see it.
#pragma once
#include "fcx_device.h"

namespace fcx {

constexpr uint32_t kTailR = 64;      // R entries up to which a tile goes to the tail kernel (one per lane)
constexpr uint32_t kTailHead = 16;   // words before the flags; word 0: the tail list's length
constexpr uint32_t kTailGrid = 5120; // k_sparse_tail's one-wave workgroups (20 per CU: 7.1 KB of LDS each)

// The tail flags of a call over nt tiles -- a byte per tile, zeroed before the call's match stage; a
// listed tile's is its R's length (2 .. kTailR) -- lie behind the nt mtok slots the call uses (the
// scratch is sized for them, sparse_tail_bytes): their place follows from what every match kernel is
// given already.  A plain store: a counter shared by every workgroup would take a returning atomic
// on one address from all eight XCDs at the end of 4 tiles in 10.  Behind the flags,
// the list of the flagged tiles (k_sparse_tail_list: one atomic per 1024 tiles).  A tile's mtok slot,
// idle until the parse, holds its R meanwhile.
__host__ __device__ inline uint32_t *sparse_tail_head(uint32_t *mtok, uint32_t nt) {
    return mtok + (uint64_t)kTileMatches * nt;
}
__host__ __device__ inline uint8_t *sparse_tail_flags(uint32_t *mtok, uint32_t nt) {
    return (uint8_t *)(sparse_tail_head(mtok, nt) + kTailHead);
}
constexpr uint64_t sparse_tail_flag_bytes(uint64_t nt) { return 4 * kTailHead + ((nt + 63) & ~63ull); }   // head + flags
__host__ __device__ inline uint32_t *sparse_tail_list(uint32_t *mtok, uint32_t nt) {
    return (uint32_t *)((uint8_t *)sparse_tail_head(mtok, nt) + sparse_tail_flag_bytes(nt));
}
constexpr uint64_t sparse_tail_bytes(uint64_t nt) { return sparse_tail_flag_bytes(nt) + 4 * nt; }
static_assert(kTailR <= kTileMatches && kTailR < 256, "R fits the tile's mtok slot, its length a byte");

// the flagged tiles into the list, then the tail kernel over it (a fixed grid; the list's length is
// read on the device)
void launch_sparse_tail(const MatchArgs &a, hipStream_t st);

}  // namespace fcx
