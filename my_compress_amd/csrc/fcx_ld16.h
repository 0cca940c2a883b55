// fcx_ld16.h — what the kernels over record runs share (fcx_verify.hip, fcx_repair.hip, fcx_digest.hip,
// fcx_find.hip, fcx_lines.hip, fcx_grep.hip, fcx_ranges.hip; DESIGN.md §1a, "run core"): the bounded 16-byte read of a
// byte range that sits anywhere, a block's length, the "no entry" mark of the entry map, and the tail of the two
// summary kernels.  Device code only, and included by those files alone: no compress-path or decoder object sees it.
#ifndef FCX_LD16_H
#define FCX_LD16_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fcx_dec_shared.h"   // kVw*
#include "fcx_device.h"       // wave_sum_u64

namespace fcx {

constexpr uint32_t kNoEntry = 0xFFFFFFFFu;   // entry_of: the record has no entry

// bytes of block k of n bytes cut into blocks of B (0 behind the end)
__device__ inline uint32_t block_len(uint64_t k, uint64_t n, uint32_t B) {
    const uint64_t o0 = k * B;
    return o0 < n ? (uint32_t)min((uint64_t)B, n - o0) : 0u;
}

// the 16 bytes at p + i of a byte range that starts at p (any alignment): two aligned 16-byte loads and
// a funnel shift.  `sh` = (address of p + i) & 15 is the same for every piece of a block, since
// pieces are 16 bytes apart.  The caller has checked that the aligned 32 bytes lie inside the block.
__device__ inline uint4 ld16_shifted(const uint8_t *a, uint32_t sh) {
    const uint4 *q = (const uint4 *)(a - sh);
    const uint4 lo = q[0];
    if (sh == 0) return lo;
    const uint4 hi = q[1];
    const uint32_t bs = sh & 3;
    uint32_t w0, w1, w2, w3, w4;
    switch (sh >> 2) {   // (uniform over the workgroup)
    case 0: w0 = lo.x; w1 = lo.y; w2 = lo.z; w3 = lo.w; w4 = hi.x; break;
    case 1: w0 = lo.y; w1 = lo.z; w2 = lo.w; w3 = hi.x; w4 = hi.y; break;
    case 2: w0 = lo.z; w1 = lo.w; w2 = hi.x; w3 = hi.y; w4 = hi.z; break;
    default: w0 = lo.w; w1 = hi.x; w2 = hi.y; w3 = hi.z; w4 = hi.w; break;
    }
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, bs), __builtin_amdgcn_alignbyte(w2, w1, bs),
                      __builtin_amdgcn_alignbyte(w3, w2, bs), __builtin_amdgcn_alignbyte(w4, w3, bs));
}

// The 16 bytes at p + i of the range [p, p + len), i + 16 <= len, sh = (address of p + i) & 15: the
// memory-safety rule of the byte-range kernels.  Through ld16_shifted where the aligned window it loads
// (32 bytes, 16 when sh is 0) lies inside the range, byte by byte otherwise (a range's head and tail):
// nothing outside the range is read.
__device__ inline uint4 ld16_bounded(const uint8_t *p, uint64_t i, uint32_t sh, uint64_t len) {
    if (i >= sh && i - sh + (sh ? 32 : 16) <= len) return ld16_shifted(p + i, sh);
    uint32_t x[4];
    for (uint32_t q = 0; q < 4; q++) {
        const uint8_t *b = p + i + 4 * q;
        x[q] = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    return make_uint4(x[0], x[1], x[2], x[3]);
}

// minimum over the 64 lanes (uniform)
__device__ inline uint64_t wave_min_u64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v = min(v, ((uint64_t)hi << 32) | lo);
    }
    return v;
}

// The tail of a summary kernel (one workgroup; every thread with its own counts): the failing blocks,
// the first of them, the blocks of another size and the failing blocks' bytes into the status words
// (kVw*, zeroed before, kVwFirst preset to ~0), with the run's records and decoded bytes.
__device__ inline void publish_verdict(uint64_t differ, uint64_t first, uint64_t sized, uint64_t bytes, uint32_t nblocks,
                                       const uint64_t *__restrict__ dec_off, uint64_t *__restrict__ words) {
    differ = wave_sum_u64(differ);
    sized = wave_sum_u64(sized);
    bytes = wave_sum_u64(bytes);
    first = wave_min_u64(first);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *w = (unsigned long long *)words;
        if (differ) {
            atomicAdd(w + kVwDiffer, (unsigned long long)differ);
            atomicAdd(w + kVwBytes, (unsigned long long)bytes);
            atomicMin(w + kVwFirst, (unsigned long long)first);
        }
        if (sized) atomicAdd(w + kVwSized, (unsigned long long)sized);
    }
    if (threadIdx.x == 0) {
        words[kVwBlocks] = nblocks;
        words[kVwDecoded] = dec_off[nblocks];
    }
}

}  // namespace fcx

#endif  // FCX_LD16_H
