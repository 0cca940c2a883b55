// fcx_sparse_filter.h — the sparse unit's repeat filter: the hash both the kernel (fcx_match.hip under
// FCX_SPARSE) and the host model (fcx_debug_sparse_filter, fcx_capi.hip) compile.
//
// One bitmap of kSfWords 32-bit words: the search's 32 KiB region less its last 512 words, which
// hold the search's lists, so the flagged keys are listed while the bitmap is still live.  A 3-byte key picks its word by key_mix and kSfK bits
// inside the word by a second multiplicative mix (the key has only 24 bits); it is inserted by one
// atomicOr of those bits and counts as flagged when every one of them was already set.  Equal keys
// pick the same word and bits, and same-word atomics serialise, so of every set of equal keys in a
// window at most one (whichever ran first) is not flagged.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FCX_SF_HD __host__ __device__
#else
#define FCX_SF_HD
#endif

namespace fcx {

constexpr uint32_t kSfWords = 7680;   // bitmap words (the region's first; 512 words stay for the lists)
#ifndef FCX_SF_K
#define FCX_SF_K 4
#endif
constexpr uint32_t kSfK = FCX_SF_K;   // bits per key (chosen by the phase timing)
static_assert(kSfK >= 2 && kSfK <= 5, "two to five bits per key");
// flagged keys per window up to which a tile stays in the sparse search (the largest
// count over the first 64 MiB of the seed-4 random stream, and what a tile at the cap costs)
constexpr uint32_t kSfFlagCap = 64;
// R, the window positions whose exact key equals a flagged one: the flagged positions themselves
// and their unflagged partners.  Covers the 64 match positions sparse_parse accepts with a
// candidate each, plus the false positives of a tile at the cap.
constexpr uint32_t kSfRCap = 256;

// 4 x the word index of a 24-bit key (its byte offset in the bitmap): key_mix, a bijection of
// Z/2^24 (only the multiplier's low 24 bits reach the product's low 24), scaled to [0, kSfWords)
// by the high half of a second 24 x 24-bit product: two multiplies and a mask.  (The second is a
// full-rate v_mul_hi_u32_u24; the first comes out as a 32-bit v_mul_lo_u32, also when written as
// __umul24: only its low 24 bits are used, so the compiler drops the key's mask and with it the
// proof that the key fits 24 bits.  DESIGN.md §4d)
FCX_SF_HD inline uint32_t sf_word_x4(uint32_t key) {
    const uint32_t h = ((key & 0xFFFFFFu) * 0x3779B1u) & 0xFFFFFFu;
    static_assert((kSfWords << 10) < (1u << 24), "a 24-bit scale");
    return (uint32_t)(((uint64_t)h * (kSfWords << 10)) >> 32) & ~3u;
}
FCX_SF_HD inline uint32_t sf_word(uint32_t key) { return sf_word_x4(key) >> 2; }
// the key's bits inside its word: the top bits of another 24 x 24-bit product
FCX_SF_HD inline uint32_t sf_bits(uint32_t key) {
    const uint32_t p = (key & 0xFFFFFFu) * 0xC2B2AFu;
    uint32_t b = (1u << (p >> 27)) | (1u << ((p >> 22) & 31u));
    if (kSfK >= 3) b |= 1u << ((p >> 17) & 31u);
    if (kSfK >= 4) b |= 1u << ((p >> 12) & 31u);
    if (kSfK >= 5) b |= 1u << ((p >> 7) & 31u);
    return b;
}

}  // namespace fcx
