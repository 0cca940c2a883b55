// fcx_regex.h — the regular expression of include/fcx.h, compiled on the host into the one block of bytes that the
// scan kernels of fcx_regex.hip stage in LDS.  Pure host code without a HIP header: the library's entry points
// (fcx_regex.hip), the command line's host path (fcx_cli_host.h) and tools/regex_host_check.cpp share it.
// DESIGN.md §9l.
//
//   parse      a POSIX ERE subset over bytes (the syntax and the refusals: include/fcx.h) into a tree; the anchors
//              are flags of the top-level alternatives, never nodes.
//   positions  Glushkov: every byte set of the tree, counted repetitions expanded, is a position with its follow
//              set; at most kRxMaxPos of them.
//   subsets    the unanchored search automaton: a state is the set of positions a match in progress may stand at,
//              plus "no byte of the line was read yet"; every step adds the first positions of the alternatives
//              without ^ (the Σ* loop), and at the line's start those with ^ too.  The delimiter leads to the start
//              state from every state.  Bytes that no position tells apart share a class from the outset.
//   minimise   Moore's refinement from (acc, acc_eol), then the classes with equal columns are merged.
#ifndef FCX_REGEX_H
#define FCX_REGEX_H

#include <algorithm>
#include <array>
#include <bitset>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_patset.h"   // fold_ascii

namespace fcx {

constexpr uint32_t kRxMaxPos = 1024;       // NFA positions after expanding the counted repetitions
constexpr uint32_t kRxMaxSubsets = 4096;   // states during subset construction
constexpr uint32_t kRxMaxCount = 255;      // n of {m,n}
// The block, in bytes: 16 header words (kRxH*), cls[256], then next[class][state] with `stride` bytes per class:
// the states rounded up to whole dwords, and to an odd number of dwords so that the classes spread over the banks.
constexpr uint32_t kRxHStates = 0, kRxHClasses = 1, kRxHStride = 2, kRxHStart = 3, kRxHDelim = 4, kRxHFlags = 5;
constexpr uint32_t kRxHAcc = 6, kRxHAccEol = 8;   // two words each
constexpr uint32_t kRxCls = 64;
constexpr uint32_t kRxNext = kRxCls + 256;
constexpr uint32_t kRxMaxStride = 4 * ((FCX_REGEX_MAX_STATES / 4) | 1);   // 68
constexpr uint32_t kRxBlockBytes = kRxNext + 256 * kRxMaxStride;          // 17728
static_assert(kRxBlockBytes % 16 == 0 && kRxNext % 16 == 0, "regex block: staged by 16 bytes");

inline uint32_t rx_stride(uint32_t states) { return 4 * (((states + 3) / 4) | 1); }

}  // namespace fcx

struct fcx_regex {
    uint32_t nstates = 0, nclasses = 0, flags = 0, start = 0, stride = 0, block_bytes = 0;
    uint8_t delim = 0x0A;
    uint64_t acc = 0, acc_eol = 0;
    alignas(16) uint8_t block[fcx::kRxBlockBytes] = {};
    uint8_t step(uint8_t state, uint8_t byte) const {
        return block[fcx::kRxNext + (uint32_t)block[fcx::kRxCls + byte] * stride + state];
    }
    // is the position whose byte led to `state` a hit?  at_end: the byte behind it is the delimiter or the run ends
    bool hit(uint8_t state, bool at_end) const { return ((acc >> state) & 1) || (at_end && ((acc_eol >> state) & 1)); }
};

namespace fcx {

typedef std::array<uint64_t, 4> RxSet;                 // a set of byte values
typedef std::bitset<kRxMaxPos + 1> RxBits;             // a set of positions; bit kRxMaxPos: at the line's start

struct RxCompiler {
    enum { LIT, CAT, ALT, STAR, PLUS, OPT, REP };
    struct Node {
        int type, a, b;      // LIT: a = index into sets; REP: b = m | n << 16 (n == 0xFFFF: unbounded)
    };
    struct Alt {
        bool bol, eol;
        int node;
    };
    struct Frag {
        bool nullable = true;
        RxBits first, last;
    };
    const uint8_t *e;
    uint32_t n, at = 0, flags;
    uint8_t d;
    std::string err;
    std::vector<Node> nodes;
    std::vector<RxSet> sets;
    std::vector<Alt> alts;
    std::vector<int> pos_set;           // per position: index into sets
    std::vector<RxBits> follow;

    RxCompiler(const uint8_t *expr, uint32_t len, uint8_t delim, uint32_t fl) : e(expr), n(len), flags(fl), d(delim) {}

    bool fail_at(uint32_t off, const char *what) {
        if (err.empty()) err = std::string(what) + " at offset " + std::to_string(off);
        return false;
    }
    bool fail(const std::string &what) {   // (what no single offset is to blame for)
        if (err.empty()) err = what;
        return false;
    }
    static bool has(const RxSet &s, uint32_t b) { return (s[b >> 6] >> (b & 63)) & 1; }
    static void put(RxSet &s, uint32_t b) { s[b >> 6] |= 1ull << (b & 63); }
    void put_folded(RxSet &s, uint32_t b) const {
        put(s, b);
        if (flags & FCX_SET_FOLD_ASCII) {
            if (b >= 0x41 && b <= 0x5A) put(s, b + 0x20);
            if (b >= 0x61 && b <= 0x7A) put(s, b - 0x20);
        }
    }
    int node(int type, int a, int b) {
        nodes.push_back(Node{type, a, b});
        return (int)nodes.size() - 1;
    }
    int lit(const RxSet &s) {
        sets.push_back(s);
        return node(LIT, (int)sets.size() - 1, 0);
    }
    // a set the expression names byte by byte: it must not hold the delimiter
    bool checked(const RxSet &s, uint32_t off) { return has(s, d) ? fail_at(off, "the delimiter in a literal or a set") : true; }
    void negate(RxSet &s) const {
        for (uint64_t &w : s) w = ~w;
        s[d >> 6] &= ~(1ull << (d & 63));
    }
    // the named classes and the shorthands leave the delimiter out
    void put_class(RxSet &s, const char *name) const {
        for (uint32_t b = 0; b < 128; b++) {
            const bool up = b >= 'A' && b <= 'Z', lo = b >= 'a' && b <= 'z', dg = b >= '0' && b <= '9';
            const bool sp = b == ' ' || (b >= 9 && b <= 13), pr = b > 32 && b < 127;
            bool in = false;
            if (!strcmp(name, "alpha")) in = up || lo;
            else if (!strcmp(name, "digit")) in = dg;
            else if (!strcmp(name, "alnum")) in = up || lo || dg;
            else if (!strcmp(name, "upper")) in = up;
            else if (!strcmp(name, "lower")) in = lo;
            else if (!strcmp(name, "space")) in = sp;
            else if (!strcmp(name, "punct")) in = pr && !(up || lo || dg);
            else if (!strcmp(name, "xdigit")) in = dg || (b >= 'A' && b <= 'F') || (b >= 'a' && b <= 'f');
            else if (!strcmp(name, "word")) in = up || lo || dg || b == '_';
            if (in && b != d) put_folded(s, b);
        }
        s[d >> 6] &= ~(1ull << (d & 63));   // (a folded letter may be the delimiter)
    }

    // [...] with at at the byte behind '['
    int parse_bracket() {
        const uint32_t open = at - 1;
        RxSet s = {};
        bool neg = false;
        if (at < n && e[at] == '^') {
            neg = true;
            at++;
        }
        bool first = true;
        for (;; first = false) {
            if (at >= n) return fail_at(open, "unterminated bracket set"), -1;
            uint32_t c = e[at];
            if (c == ']' && !first) {
                at++;
                break;
            }
            if (c == '[' && at + 1 < n && e[at + 1] == ':') {
                uint32_t q = at + 2;
                while (q + 1 < n && !(e[q] == ':' && e[q + 1] == ']')) q++;
                if (q + 1 >= n) return fail_at(at, "unterminated character class"), -1;
                const std::string name((const char *)e + at + 2, q - at - 2);
                static const char *known[] = {"alpha", "digit", "alnum", "upper", "lower", "space", "punct", "xdigit"};
                bool ok = false;
                for (const char *k : known) ok = ok || name == k;
                if (!ok) return fail_at(at, "unknown character class"), -1;
                put_class(s, name.c_str());
                at = q + 2;
                continue;
            }
            if (c == '[' && at + 1 < n && (e[at + 1] == '.' || e[at + 1] == '=')) return fail_at(at, "collating elements are not supported"), -1;
            at++;
            uint32_t hi = c;
            if (at + 1 < n && e[at] == '-' && e[at + 1] != ']') {
                hi = e[at + 1];
                if (hi == '[' && at + 2 < n && (e[at + 2] == ':' || e[at + 2] == '.' || e[at + 2] == '=')) return fail_at(at, "bad range end"), -1;
                if (hi < c) return fail_at(at - 1, "range out of order"), -1;
                at += 2;
            }
            RxSet r = {};
            for (uint32_t b = c; b <= hi; b++) put_folded(r, b);
            if (!neg && !checked(r, at - 1)) return -1;
            for (int i = 0; i < 4; i++) s[i] |= r[i];
        }
        if (neg) negate(s);
        if (s == RxSet{}) return fail_at(open, "a set that matches no byte"), -1;
        return lit(s);
    }

    // one item without its repetition; -1: error
    int parse_atom(int depth) {
        const uint32_t off = at;
        const uint8_t c = e[at++];
        RxSet s = {};
        switch (c) {
        case '(': {
            const int r = parse_alt(depth + 1);
            if (r < 0) return -1;
            if (at >= n || e[at] != ')') return fail_at(off, "unmatched ("), -1;
            at++;
            return r;
        }
        case '[': return parse_bracket();
        case '.':
            negate(s);
            return lit(s);
        case '^':
        case '$': return fail_at(off, "an anchor that is not the first or last item of a top-level alternative"), -1;
        case '*':
        case '+':
        case '?':
        case '{': return fail_at(off, "a repetition with nothing in front of it"), -1;
        case '\\': {
            if (at >= n) return fail_at(off, "a trailing backslash"), -1;
            const uint8_t x = e[at++];
            if (x == 'w' || x == 'W' || x == 's' || x == 'S') {
                put_class(s, (x | 0x20) == 'w' ? "word" : "space");
                if (x < 'a') negate(s);
                if (s == RxSet{}) return fail_at(off, "a set that matches no byte"), -1;
                return lit(s);
            }
            if (x >= '1' && x <= '9') return fail_at(off, "back-references are not supported"), -1;
            if (x == 'b' || x == 'B' || x == '<' || x == '>') return fail_at(off, "word boundaries are not supported"), -1;
            const bool punct = x > 32 && x < 127 && !((x | 0x20) >= 'a' && (x | 0x20) <= 'z') && !(x >= '0' && x <= '9');
            if (!punct) return fail_at(off, "unknown escape"), -1;
            put_folded(s, x);
            if (!checked(s, off)) return -1;
            return lit(s);
        }
        default:
            put_folded(s, c);
            if (!checked(s, off)) return -1;
            return lit(s);
        }
    }

    // a sequence up to '|', ')' or the end; at depth 0 it strips the anchors into *bol / *eol
    int parse_seq(int depth, bool *bol, bool *eol) {
        const uint32_t off = at;
        int seq = -1;
        if (depth == 0 && at < n && e[at] == '^') {
            *bol = true;
            at++;
        }
        while (at < n && e[at] != '|' && e[at] != ')') {
            if (depth == 0 && e[at] == '$' && (at + 1 == n || e[at + 1] == '|')) {
                *eol = true;
                at++;
                break;
            }
            int a = parse_atom(depth);
            if (a < 0) return -1;
            while (at < n && (e[at] == '*' || e[at] == '+' || e[at] == '?' || e[at] == '{')) {
                const uint32_t roff = at;
                const uint8_t r = e[at++];
                if (r == '*') a = node(STAR, a, 0);
                else if (r == '+') a = node(PLUS, a, 0);
                else if (r == '?') a = node(OPT, a, 0);
                else {
                    uint32_t m = 0, hi = 0;
                    bool dm = false, dh = false, comma = false;
                    while (at < n && e[at] >= '0' && e[at] <= '9' && m <= kRxMaxCount) m = 10 * m + (e[at++] - '0'), dm = true;
                    if (at < n && e[at] == ',') {
                        comma = true;
                        at++;
                        while (at < n && e[at] >= '0' && e[at] <= '9' && hi <= kRxMaxCount) hi = 10 * hi + (e[at++] - '0'), dh = true;
                    }
                    if (!dm || at >= n || e[at] != '}') return fail_at(roff, "a malformed repetition count"), -1;
                    at++;
                    if (!comma) hi = m;
                    else if (!dh) hi = 0xFFFF;
                    if (m > kRxMaxCount || (hi != 0xFFFF && (hi > kRxMaxCount || hi < m))) return fail_at(roff, "a repetition count out of range"), -1;
                    // (a count of zero builds no position, so the position limit would not bound what nests over it)
                    if (hi == 0) return fail_at(roff, "a repetition count of zero"), -1;
                    a = node(REP, a, (int)(m | hi << 16));
                }
            }
            seq = seq < 0 ? a : node(CAT, seq, a);
        }
        if (seq < 0) {
            if (depth == 0 && (*bol || *eol)) return fail_at(off, "the expression matches the empty string"), -1;
            return fail_at(off, "an empty alternative"), -1;
        }
        return seq;
    }

    int parse_alt(int depth) {
        int alt = -1;
        for (;;) {
            bool bol = false, eol = false;
            const int s = parse_seq(depth, &bol, &eol);
            if (s < 0) return -1;
            if (depth == 0) alts.push_back(Alt{bol, eol, s});
            alt = alt < 0 ? s : node(ALT, alt, s);
            if (at < n && e[at] == '|') {
                at++;
                continue;
            }
            if (depth == 0 && at < n) return fail_at(at, "unmatched )"), -1;
            return alt;
        }
    }

    // ---- Glushkov ----
    void link(const RxBits &from, const RxBits &to) {
        for (uint32_t p = 0; p < pos_set.size(); p++)
            if (from[p]) follow[p] |= to;
    }
    Frag cat(const Frag &a, const Frag &b) {
        Frag r;
        link(a.last, b.first);
        r.first = a.nullable ? a.first | b.first : a.first;
        r.last = b.nullable ? a.last | b.last : b.last;
        r.nullable = a.nullable && b.nullable;
        return r;
    }
    Frag loop(Frag x, bool nullable) {
        link(x.last, x.first);
        x.nullable = x.nullable || nullable;
        return x;
    }
    Frag build(int k) {
        Frag r;
        if (!err.empty()) return r;
        const Node nd = nodes[k];
        switch (nd.type) {
        case LIT:
            if (pos_set.size() >= kRxMaxPos) {
                err = "more than 1024 positions after expanding the repetitions";
                return r;
            }
            r.nullable = false;
            r.first[pos_set.size()] = r.last[pos_set.size()] = true;
            pos_set.push_back(nd.a);
            follow.emplace_back();
            return r;
        case CAT: {
            const Frag a = build(nd.a);
            return cat(a, build(nd.b));
        }
        case ALT: {
            const Frag a = build(nd.a), b = build(nd.b);
            r.nullable = a.nullable || b.nullable;
            r.first = a.first | b.first;
            r.last = a.last | b.last;
            return r;
        }
        case STAR: return loop(build(nd.a), true);
        case PLUS: return loop(build(nd.a), false);
        case OPT:
            r = build(nd.a);
            r.nullable = true;
            return r;
        default: {
            const uint32_t m = (uint32_t)nd.b & 0xFFFF, hi = (uint32_t)nd.b >> 16;
            for (uint32_t i = 0; i + 1 < m && err.empty(); i++) r = cat(r, build(nd.a));
            if (hi == 0xFFFF) return cat(r, loop(build(nd.a), m == 0));
            if (m) r = cat(r, build(nd.a));
            for (uint32_t i = m; i < hi && err.empty(); i++) {
                Frag o = build(nd.a);
                o.nullable = true;
                r = cat(r, o);
            }
            return r;
        }
        }
    }

    // false: err says what is wrong (and names the offset where one is to blame)
    bool compile(fcx_regex *re) {
        if (parse_alt(0) < 0) return false;
        RxBits first_free, first_all, acc_pos, eol_pos;
        for (const Alt &a : alts) {
            const Frag f = build(a.node);
            if (!err.empty()) return false;
            if (f.nullable) return fail("the expression matches the empty string");
            first_all |= f.first;
            if (!a.bol) first_free |= f.first;
            (a.eol ? eol_pos : acc_pos) |= f.last;
        }
        const uint32_t np = (uint32_t)pos_set.size();
        // byte classes from the positions' sets; the delimiter has its own (no position holds it)
        std::map<std::vector<bool>, uint32_t> sig_class;
        uint8_t cls0[256];
        std::vector<uint8_t> rep;
        for (uint32_t b = 0; b < 256; b++) {
            std::vector<bool> sig(np + 1);
            for (uint32_t p = 0; p < np; p++) sig[p] = has(sets[pos_set[p]], b);
            sig[np] = b == d;
            auto it = sig_class.find(sig);
            if (it == sig_class.end()) {
                it = sig_class.emplace(sig, (uint32_t)rep.size()).first;
                rep.push_back((uint8_t)b);
            }
            cls0[b] = (uint8_t)it->second;
        }
        const uint32_t nc0 = (uint32_t)rep.size();
        std::vector<RxBits> pos_of(nc0);
        for (uint32_t c = 0; c < nc0; c++)
            for (uint32_t p = 0; p < np; p++)
                if (has(sets[pos_set[p]], rep[c])) pos_of[c][p] = true;
        // subsets
        auto less = [](const RxBits &a, const RxBits &b) { return memcmp(&a, &b, sizeof(RxBits)) < 0; };
        std::map<RxBits, uint32_t, decltype(less)> ids(less);
        std::vector<RxBits> states;
        std::vector<std::vector<uint32_t>> next;
        RxBits init;
        init[kRxMaxPos] = true;
        ids.emplace(init, 0);
        states.push_back(init);
        for (uint32_t s = 0; s < states.size(); s++) {
            const RxBits cur = states[s];
            RxBits cand = cur[kRxMaxPos] ? first_all : first_free;
            for (uint32_t p = 0; p < np; p++)
                if (cur[p]) cand |= follow[p];
            next.emplace_back(nc0);
            for (uint32_t c = 0; c < nc0; c++) {
                const RxBits to = rep[c] == d ? init : (cand & pos_of[c]);
                auto it = ids.find(to);
                if (it == ids.end()) {
                    if (states.size() >= kRxMaxSubsets) return fail("more than 4096 states during subset construction");
                    it = ids.emplace(to, (uint32_t)states.size()).first;
                    states.push_back(to);
                }
                next[s][c] = it->second;
            }
        }
        // Moore
        const uint32_t ns = (uint32_t)states.size();
        std::vector<uint32_t> part(ns);
        for (uint32_t s = 0; s < ns; s++) part[s] = ((states[s] & acc_pos).any() ? 1u : 0u) | ((states[s] & eol_pos).any() ? 2u : 0u);
        uint32_t nparts = 0;
        for (;;) {
            std::map<std::vector<uint32_t>, uint32_t> seen;
            std::vector<uint32_t> np2(ns);
            for (uint32_t s = 0; s < ns; s++) {
                std::vector<uint32_t> sig(nc0 + 1);
                sig[0] = part[s];
                for (uint32_t c = 0; c < nc0; c++) sig[c + 1] = part[next[s][c]];
                np2[s] = seen.emplace(sig, (uint32_t)seen.size()).first->second;
            }
            const bool stable = seen.size() == nparts;
            nparts = (uint32_t)seen.size();
            part = np2;
            if (stable) break;
        }
        if (nparts > FCX_REGEX_MAX_STATES)
            return fail("more than 64 states after minimisation (" + std::to_string(nparts) + ")");
        std::vector<uint32_t> of_part(nparts);
        for (uint32_t s = ns; s-- > 0;) of_part[part[s]] = s;
        // classes with equal columns
        std::map<std::vector<uint8_t>, uint32_t> cols;
        std::vector<std::vector<uint8_t>> col_of;
        uint8_t merged[256];
        for (uint32_t c = 0; c < nc0; c++) {
            std::vector<uint8_t> col(nparts);
            for (uint32_t q = 0; q < nparts; q++) col[q] = (uint8_t)part[next[of_part[q]][c]];
            auto it = cols.find(col);
            if (it == cols.end()) {
                it = cols.emplace(col, (uint32_t)col_of.size()).first;
                col_of.push_back(col);
            }
            merged[c] = (uint8_t)it->second;
        }
        *re = fcx_regex();
        re->nstates = nparts;
        re->nclasses = (uint32_t)col_of.size();
        re->flags = flags;
        re->delim = d;
        re->start = part[0];
        re->stride = rx_stride(nparts);
        for (uint32_t q = 0; q < nparts; q++) {
            if ((states[of_part[q]] & acc_pos).any()) re->acc |= 1ull << q;
            if ((states[of_part[q]] & eol_pos).any()) re->acc_eol |= 1ull << q;
        }
        uint32_t *h = (uint32_t *)re->block;
        h[kRxHStates] = re->nstates;
        h[kRxHClasses] = re->nclasses;
        h[kRxHStride] = re->stride;
        h[kRxHStart] = re->start;
        h[kRxHDelim] = d;
        h[kRxHFlags] = flags;
        memcpy(h + kRxHAcc, &re->acc, 8);
        memcpy(h + kRxHAccEol, &re->acc_eol, 8);
        for (uint32_t b = 0; b < 256; b++) re->block[kRxCls + b] = merged[cls0[b]];
        for (uint32_t c = 0; c < re->nclasses; c++)
            for (uint32_t q = 0; q < re->stride; q++)   // (the padding repeats the last state: every byte of a row is a state)
                re->block[kRxNext + c * re->stride + q] = col_of[c][std::min(q, nparts - 1)];
        re->block_bytes = (kRxNext + re->nclasses * re->stride + 15) & ~15u;
        return true;
    }
};

// "" or what is wrong with the arguments
inline std::string regex_compile(fcx_regex *re, const uint8_t *expr, uint32_t len, uint8_t delim, uint32_t flags) {
    if (!re || !expr) return "NULL argument";
    if (flags & ~FCX_SET_FOLD_ASCII) return "unknown flag bits";
    if (len < 1 || len > FCX_REGEX_MAX_PATTERN) return "expression length outside [1, FCX_REGEX_MAX_PATTERN]";
    RxCompiler c(expr, len, delim, flags);
    if (!c.compile(re)) return c.err;
    return "";
}

}  // namespace fcx

#endif  // FCX_REGEX_H
