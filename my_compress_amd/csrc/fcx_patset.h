// fcx_patset.h — the pattern set of include/fcx.h, compiled on the host into the one block of words that
// k_sscan (fcx_set.hip) stages in LDS.  Pure host code without a HIP header: the library's entry points
// (fcx_set.hip), the command line's host path (fcx_cli_host.h) and tools/set_host_check.cpp share it.
// DESIGN.md §9j.
#ifndef FCX_PATSET_H
#define FCX_PATSET_H

#include <cstdint>
#include <cstring>

#include "fcx.h"

namespace fcx {

// The block, in dwords: 4 header words (npat, min_len, max_len, flags), per pattern one word
// len | first dword of its bytes << 16, the tables T0 and T1 (256 u64 each: bit k of T0[b] iff pat_k[0] == b,
// of T1[b] iff len_k < 2 or pat_k[1] == b), then the folded pattern bytes, each pattern zero-padded to a
// whole dword so that the full compare reads aligned words.
constexpr uint32_t kPsHead = 4;
constexpr uint32_t kPsMeta = kPsHead;                                  // 64 words
constexpr uint32_t kPsT0 = kPsMeta + FCX_SET_MAX_PATTERNS;             // 512 words (8-byte aligned: 68 * 4)
constexpr uint32_t kPsT1 = kPsT0 + 512;
constexpr uint32_t kPsPat = kPsT1 + 512;
constexpr uint32_t kPsPatWords = (FCX_SET_MAX_BYTES + 3 * FCX_SET_MAX_PATTERNS) / 4;   // 1072: every pattern padded
constexpr uint32_t kPsWords = kPsPat + kPsPatWords;                    // 2164 words, 8656 bytes
static_assert(kPsT0 % 2 == 0 && kPsWords % 4 == 0, "pattern set block: the tables are u64, the block goes by 16 bytes");

inline uint8_t fold_ascii(uint8_t b) { return b >= 0x41 && b <= 0x5A ? (uint8_t)(b + 0x20) : b; }

}  // namespace fcx

struct fcx_pattern_set {
    uint32_t npat = 0, min_len = 0, max_len = 0, flags = 0;
    uint32_t len[FCX_SET_MAX_PATTERNS] = {};
    uint32_t off[FCX_SET_MAX_PATTERNS] = {};   // byte offset of pattern k in `block`'s pattern area
    alignas(16) uint32_t block[fcx::kPsWords] = {};
    const uint8_t *pat(uint32_t k) const { return (const uint8_t *)(block + fcx::kPsPat) + off[k]; }
    uint8_t fold(uint8_t b) const { return (flags & FCX_SET_FOLD_ASCII) ? fcx::fold_ascii(b) : b; }
    // does a (folded) pattern hold the byte b?
    bool holds(uint8_t b) const {
        for (uint32_t k = 0; k < npat; k++)
            if (memchr(pat(k), b, len[k])) return true;
        return false;
    }
};

namespace fcx {

// nullptr, or what is wrong with the arguments
inline const char *patset_compile(fcx_pattern_set *s, const uint8_t *bytes, const uint32_t *lens, uint32_t npat, uint32_t flags) {
    if (!s || !bytes || !lens) return "NULL argument";
    if (npat < 1 || npat > FCX_SET_MAX_PATTERNS) return "number of patterns outside [1, FCX_SET_MAX_PATTERNS]";
    if (flags & ~FCX_SET_FOLD_ASCII) return "unknown flag bits";
    uint64_t sum = 0;
    for (uint32_t k = 0; k < npat; k++) {
        if (lens[k] < 1 || lens[k] > FCX_FIND_MAX_PATTERN) return "pattern length outside [1, FCX_FIND_MAX_PATTERN]";
        sum += lens[k];
    }
    if (sum > FCX_SET_MAX_BYTES) return "the patterns' bytes exceed FCX_SET_MAX_BYTES";
    *s = fcx_pattern_set();
    s->npat = npat;
    s->flags = flags;
    s->min_len = ~0u;
    uint8_t *area = (uint8_t *)(s->block + kPsPat);
    uint64_t *t0 = (uint64_t *)(s->block + kPsT0), *t1 = (uint64_t *)(s->block + kPsT1);
    uint32_t at = 0;
    for (uint32_t k = 0; k < npat; k++) {
        const uint32_t n = lens[k];
        s->len[k] = n;
        s->off[k] = at;
        s->min_len = n < s->min_len ? n : s->min_len;
        s->max_len = n > s->max_len ? n : s->max_len;
        for (uint32_t i = 0; i < n; i++) area[at + i] = s->fold(bytes[i]);
        s->block[kPsMeta + k] = n | (at / 4) << 16;
        t0[area[at]] |= 1ull << k;
        if (n < 2) {
            for (uint32_t b = 0; b < 256; b++) t1[b] |= 1ull << k;
        } else {
            t1[area[at + 1]] |= 1ull << k;
        }
        bytes += n;
        at += (n + 3) & ~3u;
    }
    s->block[0] = npat;
    s->block[1] = s->min_len;
    s->block[2] = s->max_len;
    s->block[3] = flags;
    return nullptr;
}

}  // namespace fcx

#endif  // FCX_PATSET_H
