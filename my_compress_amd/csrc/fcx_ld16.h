// fcx_ld16.h — the unaligned 16-byte load the byte-range kernels share: k_vcompare (fcx_verify.hip) and
// the repair kernels (fcx_repair.hip).  Device code only.
#ifndef FCX_LD16_H
#define FCX_LD16_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fcx {

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

}  // namespace fcx

#endif  // FCX_LD16_H
