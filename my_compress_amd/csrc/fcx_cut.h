// fcx_cut.h — the cut of include/fcx.h, compiled on the host: GNU cut's LIST into the selection table that
// k_kmark (fcx_cut.hip) stages in LDS, and the rule itself over bytes in host memory.  Pure host code without a
// HIP header, so that the library's entry points and a host-only caller can share it.  DESIGN.md §9m.
#ifndef FCX_CUT_H
#define FCX_CUT_H

#include <cstdint>
#include <string>

#include "fcx.h"

namespace fcx {

// Columns are judged through sel(min(k, kCutSat)): every column above FCX_CUT_MAX_COLUMN is selected or not with
// all the others, so a tick count that saturates at kCutSat loses nothing.  (A separator needs k > mn beside
// sel(k): mn <= kCutSat, and the count distinguishes kCutSat from kCutSat + 1 ticks' worth of columns.)
constexpr uint32_t kCutSat = FCX_CUT_MAX_COLUMN + 1;      // 4097
constexpr uint32_t kCutSelWords = (kCutSat + 1 + 31) / 32 + 3;   // bits 0 .. 4097, padded to 16 bytes: 132 words
static_assert(kCutSelWords % 4 == 0, "the selection table goes by 16 bytes");

}  // namespace fcx

struct fcx_cut {
    uint32_t mode = 0, flags = 0, mn = 0, open_end = 0;
    uint8_t sep = 0, delim = 0;
    alignas(16) uint32_t sel[fcx::kCutSelWords] = {};   // bit k: column k is selected, 1 <= k <= kCutSat
    bool selected(uint64_t k) const {
        const uint32_t i = k < fcx::kCutSat ? (uint32_t)k : fcx::kCutSat;
        return (sel[i >> 5] >> (i & 31)) & 1u;
    }
};

namespace fcx {

// "" or what is wrong with the arguments, naming the offset in LIST where there is one
inline std::string cut_compile(fcx_cut *c, const char *list, uint32_t len, uint32_t mode, uint8_t sep, uint8_t delim, uint32_t flags) {
    if (!c || (!list && len)) return "NULL argument";
    if (mode != FCX_CUT_FIELDS && mode != FCX_CUT_BYTES) return "mode must be FCX_CUT_FIELDS or FCX_CUT_BYTES";
    if (flags & ~FCX_CUT_COMPLEMENT) return "unknown flag bits";
    if (mode == FCX_CUT_FIELDS && sep == delim) return "the separator is the delimiter";
    *c = fcx_cut();
    c->mode = mode;
    c->flags = flags;
    c->sep = mode == FCX_CUT_FIELDS ? sep : 0;
    c->delim = delim;
    const auto at = [](uint32_t i, const char *why) { return "LIST offset " + std::to_string(i) + ": " + why; };
    if (len == 0) return at(0, "an empty list");
    const auto set_range = [&](uint32_t lo, uint32_t hi) {
        for (uint32_t k = lo; k <= hi; k++) c->sel[k >> 5] |= 1u << (k & 31);
    };
    uint32_t i = 0;
    for (;;) {
        // one item: N, N-M, N- or -M
        const uint32_t item = i;
        uint64_t v[2] = {0, 0};
        bool have[2] = {false, false}, dash = false;
        for (int side = 0; side < 2; side++) {
            const uint32_t num = i;
            while (i < len && list[i] >= '0' && list[i] <= '9') {
                if (v[side] <= kCutSat) v[side] = 10 * v[side] + (uint32_t)(list[i] - '0');
                have[side] = true;
                i++;
            }
            if (have[side] && v[side] == 0) return at(num, "columns are numbered from 1");
            if (side == 0 && i < len && list[i] == '-') {
                dash = true;
                i++;
            } else {
                break;
            }
        }
        if (i < len && list[i] != ',') return at(i, "a byte that is no digit, '-' or ','");
        if (!have[0] && !have[1]) return at(item, dash ? "a range without a number" : "an empty item");
        const uint32_t lo = have[0] ? (uint32_t)v[0] : 1;
        if (dash && !have[1]) {   // N-: its start may be the first column above the maximum, no later one
            if (lo > kCutSat) return at(item, "an open range starts above FCX_CUT_MAX_COLUMN + 1");
            set_range(lo, kCutSat);
            c->open_end = 1;
        } else {
            const uint32_t hi = dash ? (uint32_t)v[1] : lo;
            if (lo > FCX_CUT_MAX_COLUMN || hi > FCX_CUT_MAX_COLUMN) return at(item, "a column above FCX_CUT_MAX_COLUMN");
            if (hi < lo) return at(item, "a descending range");
            set_range(lo, hi);
        }
        if (i == len) break;
        i++;   // the comma
        if (i == len) return at(i, "an empty item");
    }
    if (flags & FCX_CUT_COMPLEMENT)
        for (uint32_t k = 1; k <= kCutSat; k++) c->sel[k >> 5] ^= 1u << (k & 31);
    for (uint32_t k = 1; k <= kCutSat && !c->mn; k++)
        if (c->selected(k)) c->mn = k;
    if (!c->mn) return at(0, "the complement of the list selects no column");
    return "";
}

// The rule over n bytes in host memory, continuing a text: *ticks is the open line's tick count (saturated; 0
// starts a text).  Kept bytes are appended to out; stats (FCX_CUT_STATS values, may be null) advance, all but
// the groups.
inline void cut_host_bytes(const fcx_cut &c, const uint8_t *p, uint64_t n, uint32_t *ticks, std::string *out, uint64_t *stats) {
    const bool fields = c.mode == FCX_CUT_FIELDS;
    uint32_t t = *ticks;
    uint64_t kept = 0, nd = 0, ns = 0, nk = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t b = p[i];
        bool keep;
        if (b == c.delim) {
            keep = true;
            nd++;
            t = 0;
        } else if (fields && b == c.sep) {
            const uint32_t k = t + 2;
            keep = c.selected(k) && k > c.mn;
            ns++;
            nk += keep;
            t = t < kCutSat ? t + 1 : kCutSat;
        } else {
            keep = c.selected(t + 1);
            if (!fields) t = t < kCutSat ? t + 1 : kCutSat;
        }
        if (keep) {
            if (out) out->push_back((char)b);
            kept++;
        }
    }
    *ticks = t;
    if (stats) {
        stats[0] += kept;
        stats[1] += n;
        stats[2] += nd;
        stats[3] += ns;
        stats[4] += nk;
    }
}

}  // namespace fcx

#endif  // FCX_CUT_H
