// fcx_crc32.h — CRC-32/ISO-HDLC (zlib's crc32) on the host: the table-driven sum, the GF(2) arithmetic
// behind it and zlib's combine.  Host code only, header-only: the mirror of the device digest
// (fcx_digest.hip, whose tables are made here), the FCXD file (fcx_digest_file.h) and the command line's
// no-device path (fcx_cli_host.h).  DESIGN.md §9f.
//
// Polynomials are reflected: bit 31 is x^0, P = 0xEDB88320.  raw(M) = M(x) x^32 mod P is the sum with
// init and xorout 0; it is linear, raw(A | B) = shift(raw(A), |B|) ^ raw(B) with shift(c, m) = c x^(8m)
// mod P, and crc32(M) = raw(M) ^ shift(0xFFFFFFFF, |M|) ^ 0xFFFFFFFF.
#ifndef FCX_CRC32_H
#define FCX_CRC32_H

#include <cstdint>

namespace fcx_crc {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kOne = 0x80000000u;    // x^0
constexpr uint32_t kX8 = 0x00800000u;     // x^8: one byte further

// a b mod P
inline uint32_t mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (kOne >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? kPoly : 0u);
    }
    return p;
}

// x^(8m) mod P: what m bytes further multiplies a remainder by
inline uint32_t xpow8(uint64_t m) {
    uint32_t p = kOne, sq = kX8;
    for (; m; m >>= 1) {
        if (m & 1) p = mul(p, sq);
        sq = mul(sq, sq);
    }
    return p;
}

inline uint32_t shift(uint32_t c, uint64_t m) { return mul(c, xpow8(m)); }

struct Table {
    uint32_t t[256];
    Table() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? kPoly : 0u);
            t[i] = c;
        }
    }
};
inline const uint32_t *table() {
    static const Table T;
    return T.t;
}

// zlib's crc32(crc, p, n): crc32(0, p, n) is the CRC-32 of the n bytes, and the sum continues
inline uint32_t crc32(uint32_t crc, const uint8_t *p, uint64_t n) {
    const uint32_t *t = table();
    crc = ~crc;
    for (uint64_t i = 0; i < n; i++) crc = t[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
    return ~crc;
}

// zlib's crc32_combine: the CRC-32 of A | B from those of A and B and |B|
inline uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return shift(crc_a, len_b) ^ crc_b; }

// the CRC-32 of len copies of one byte, without the bytes
inline uint32_t crc32_fill(uint8_t v, uint64_t len) {
    const uint32_t *t = table();
    uint32_t r = 0, x = kOne;   // raw of the m copies so far, x^(8m)
    for (int b = 63; b >= 0; b--) {
        r = mul(r, x) ^ r;
        x = mul(x, x);
        if ((len >> b) & 1) {
            r = t[(r ^ v) & 0xFFu] ^ (r >> 8);
            x = mul(x, kX8);
        }
    }
    return r ^ mul(0xFFFFFFFFu, x) ^ 0xFFFFFFFFu;
}

}  // namespace fcx_crc

#endif  // FCX_CRC32_H
