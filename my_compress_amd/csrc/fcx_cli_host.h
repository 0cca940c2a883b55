// fcx_cli_host.h — the command line's no-device paths over an FCX7 file: the host decoder
// (fcx_decode.cpp) record by record, for the whole decompress, --list, --range, --compare, --repair, --digest, --find,
// --count-lines, --lines, --grep, --find-set, --grep-set, the context grep (--invert, --before, --after) and --grep-regex.  Host code
// only (stdio and fcx_decompress_block), so it also builds into stand-alone programs
// (tools/range_host_check.cpp, tools/compare_host_check.cpp, tools/repair_host_check.cpp, tools/digest_host_check.cpp,
// tools/find_host_check.cpp, tools/lines_host_check.cpp, tools/grep_host_check.cpp, tools/set_host_check.cpp, tools/context_host_check.cpp,
// tools/regex_host_check.cpp), and --cut-fields / --cut-bytes (tools/cut_host_check.cpp).
#ifndef FCX_CLI_HOST_H
#define FCX_CLI_HOST_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_crc32.h"
#include "fcx_cut.h"
#include "fcx_digest_file.h"
#include "fcx_patset.h"
#include "fcx_regex.h"
#include "fcx_repair_file.h"

namespace fcx_cli {

// "OFF:LEN", two unsigned decimal numbers; false for anything else
inline bool parse_range(const char *s, uint64_t *off, uint64_t *len) {
    uint64_t v[2];
    for (int i = 0; i < 2; i++) {
        if (*s < '0' || *s > '9') return false;
        uint64_t x = 0;
        for (; *s >= '0' && *s <= '9'; s++) {
            if (x > (UINT64_MAX - (uint64_t)(*s - '0')) / 10) return false;
            x = 10 * x + (uint64_t)(*s - '0');
        }
        v[i] = x;
        if (*s != (i == 0 ? ':' : '\0')) return false;
        s++;
    }
    *off = v[0];
    *len = v[1];
    return true;
}

// The nblocks records behind the header of an FCX7 file, each through the host decoder:
// fn(k, payload bytes, decoded bytes, their count) -> false ends the walk early.  0, or -1 after a
// message on stderr (a record past the end of the file, a malformed block).
template <typename Fn>
int host_each_record(FILE *fin, uint16_t nblocks, Fn fn) {
    std::vector<uint8_t> payload, plain(FCX_MAX_BLOCK_BYTES + 8);
    // bytes left in the file bound every record length before anything is sized from it
    const long here = ftell(fin);
    uint64_t left = UINT64_MAX;
    if (here >= 0 && fseek(fin, 0, SEEK_END) == 0) {
        const long end = ftell(fin);
        if (end >= here) left = (uint64_t)(end - here);
        if (fseek(fin, here, SEEK_SET) != 0) return -1;
    }
    for (uint32_t b = 0; b < nblocks; b++) {
        uint32_t sz = 0;
        if (left < 4 || fread(&sz, 4, 1, fin) != 1) return -1;
        if (left != UINT64_MAX) left -= 4;
        if (sz > left) {
            fprintf(stderr, "block %u: record of %u bytes runs past the end of the file\n", b + 1, sz);
            return -1;
        }
        if (left != UINT64_MAX) left -= sz;
        payload.resize(sz);
        if (fread(payload.data(), 1, sz, fin) != sz) return -1;
        const int64_t n = fcx_decompress_block(payload.data(), sz, plain.data(), plain.size());
        if (n < 0) {
            fprintf(stderr, "block %u: %s\n", b + 1, n == FCX_ERR_FORMAT ? "malformed" : "decode error");
            return -1;
        }
        if (!fn(b, sz, (const uint8_t *)plain.data(), (uint64_t)n)) break;
    }
    return 0;
}

inline void list_line(uint64_t k, uint64_t comp, uint64_t dec, uint64_t dec_off) {
    printf("record %llu: compressed %llu bytes, decoded %llu bytes, decoded offset %llu\n", (unsigned long long)k,
           (unsigned long long)comp, (unsigned long long)dec, (unsigned long long)dec_off);
}
inline void list_totals(uint64_t records, uint64_t comp, uint64_t dec) {
    printf("records = %llu, compressed bytes = %llu, decoded bytes = %llu\n", (unsigned long long)records,
           (unsigned long long)comp, (unsigned long long)dec);
}

// --list without a device
inline int host_list(FILE *fin, uint16_t nblocks) {
    uint64_t pos = 0, comp = 0, nrec = 0;
    const int r = host_each_record(fin, nblocks, [&](uint32_t k, uint32_t sz, const uint8_t *, uint64_t n) {
        list_line(k, sz, n, pos);
        pos += n;
        comp += sz;
        nrec++;
        return true;
    });
    if (r) return r;
    list_totals(nrec, comp, pos);
    return 0;
}

// --range without a device: the decoded bytes [off, off + len) to fout; records behind the range
// are not read
inline int host_range(FILE *fin, FILE *fout, uint16_t nblocks, uint64_t off, uint64_t len, uint64_t *written) {
    const uint64_t end = len < UINT64_MAX - off ? off + len : UINT64_MAX;
    uint64_t pos = 0, out = 0;
    bool io_ok = true;
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        const uint64_t a = off > pos ? off - pos : 0, b = end - pos < n ? end - pos : n;   // this record's part
        if (a < b) {
            io_ok = fwrite(plain + a, 1, (size_t)(b - a), fout) == b - a;
            out += b - a;
        }
        pos += n;
        return io_ok && pos < end;
    });
    if (r) return r;
    if (!io_ok) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    *written = out;
    return 0;
}

// ---- --compare / --verify: the printout, the same on the GPU and on the host ----
inline void verify_line(uint64_t k, uint64_t dec, uint64_t blen, uint64_t first_diff) {
    printf("block %llu: decoded %llu of %llu bytes, first difference at %llu\n", (unsigned long long)k,
           (unsigned long long)dec, (unsigned long long)blen, (unsigned long long)first_diff);
}
inline void verify_extra(uint64_t extra) {
    printf("original: %llu bytes after the last block\n", (unsigned long long)extra);
}
// the verdict: 0 (OK) when no block differs and the original has no bytes left, else 1 (FAIL)
inline int verify_totals(uint64_t bad, uint64_t blocks, uint64_t bytes) {
    const bool ok = bad == 0 && bytes == 0;
    printf("verify: %llu of %llu blocks differ, %llu input bytes in them [%s]\n", (unsigned long long)bad,
           (unsigned long long)blocks, (unsigned long long)bytes, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}

// --compare without a device: every record through the host decoder against its block of `block`
// bytes of forig.  A record the original has no bytes for differs (block length 0); original bytes
// behind the last record are reported and fail the verdict.  stats as fcx_verify_stream's.  Returns
// the verdict (0 / 1), or -1 after a message (a damaged record).
inline int host_compare(FILE *fin, FILE *forig, uint16_t nblocks, uint32_t block, uint64_t *stats) {
    std::vector<uint8_t> orig(block);
    uint64_t s[6] = {0, 0, UINT64_MAX, 0, 0, 0};
    const int r = host_each_record(fin, nblocks, [&](uint32_t k, uint32_t, const uint8_t *plain, uint64_t n) {
        const size_t blen = fread(orig.data(), 1, block, forig);
        const uint64_t m = n < blen ? n : blen;
        uint64_t fd = 0;
        while (fd < m && plain[fd] == orig[fd]) fd++;
        const bool differs = fd < m || n != blen || blen == 0;
        s[0]++;
        s[3] += n != blen;
        s[5] += n;
        if (differs) {
            if (blen == 0) fd = 0;
            verify_line(k, n, blen, fd);
            if (s[1]++ == 0) s[2] = k;
            s[4] += blen;
        }
        return true;
    });
    if (r) return r;
    uint64_t extra = 0;
    for (size_t g; (g = fread(orig.data(), 1, block, forig)) > 0;) extra += g;
    if (extra) {
        verify_extra(extra);
        s[4] += extra;
    }
    if (stats) memcpy(stats, s, sizeof(s));
    return verify_totals(s[1], s[0], s[4]);
}

// ---- --repair: the printout, and the FCXR file over stdio ----
inline void repair_totals(uint64_t entries, uint64_t data_bytes, uint64_t records) {
    printf("repair: %llu entries, %llu data bytes for %llu blocks\n", (unsigned long long)entries,
           (unsigned long long)data_bytes, (unsigned long long)records);
}
inline int64_t stdio_read(void *u, uint8_t *buf, uint64_t cap) {
    FILE *f = (FILE *)u;
    const size_t n = fread(buf, 1, (size_t)cap, f);
    return ferror(f) ? -1 : (int64_t)n;
}
inline int stdio_write(void *u, const uint8_t *buf, uint64_t n) { return fwrite(buf, 1, (size_t)n, (FILE *)u) == n ? 0 : -1; }
// the reason a sidecar file's reader or writer gave, to stderr; -1
template <typename T>
inline int say_err(const T &x) {
    fprintf(stderr, "fcx: %s\n", x.err.c_str());
    return -1;
}
// Record k's entry of F (null: no repair file) against the dlen bytes the record decodes to.  1: *e and
// *raw, *rlen = the bytes the entry makes of the record; 0: none, *rlen = dlen; -1 after F's message;
// -2: the entry keeps more than the record decodes to (the message is the caller's).
inline int host_entry(fcx_repair_file::Reader *F, uint32_t k, uint64_t dlen, fcx_repair_entry *e, const uint8_t **raw,
                      uint64_t *rlen) {
    *rlen = dlen;
    const int g = F ? F->next(k, (uint64_t)k + 1, e, raw) : 0;
    if (g < 0) return say_err(*F);
    if (g && e->from > dlen) return -2;
    if (g) *rlen = (uint64_t)e->from + e->len;
    return g;
}

// --compare --repair without a device: the FCXR file of the FCX7 records behind the header of fin
// against forig, to frep; the bytes fcx_repair_build_stream writes.  A record the original has no
// bytes for, or original bytes behind the last record, cannot be expressed: -1 after a message, as for
// a damaged record.  stats: FCX_REPAIR_FILE_STATS values.
inline int host_repair_build(FILE *fin, FILE *forig, uint16_t nblocks, uint32_t block, FILE *frep, uint64_t *stats) {
    fcx_repair_file::Writer W(stdio_write, frep);
    if (W.begin('7', block)) return say_err(W);
    std::vector<uint8_t> orig(block);
    uint64_t n = 0, records = 0;
    bool ok = true;
    const int r = host_each_record(fin, nblocks, [&](uint32_t k, uint32_t, const uint8_t *plain, uint64_t dlen) {
        const size_t blen = fread(orig.data(), 1, block, forig);
        if (blen == 0 || n != (uint64_t)k * block) {   // (a block before this one was short)
            fprintf(stderr, "fcx: repair: the original has no bytes for record %u\n", k);
            return ok = false;
        }
        fcx_repair_entry e;
        if (fcx_repair_file::plan_entry(k, plain, dlen, orig.data(), blen, &e) && W.add(e, orig.data() + e.from))
            return ok = say_err(W) == 0;
        n += blen;
        records++;
        return true;
    });
    if (r || !ok) return -1;
    if (fread(orig.data(), 1, 1, forig)) {
        fprintf(stderr, "fcx: repair: the original has bytes after the last record\n");
        return -1;
    }
    if (W.finish(n, records)) return say_err(W);
    const uint64_t s[FCX_REPAIR_FILE_STATS] = {n, records, W.entries, W.data_bytes};
    if (stats) memcpy(stats, s, sizeof(s));
    return 0;
}

// decompress with --repair without a device: every FCX7 record through the host decoder, its entry
// applied, to fout; the checks of fcx_repair_apply_stream.  *written: bytes written.
inline int host_repair_apply(FILE *fin, FILE *frep, FILE *fout, uint16_t nblocks, uint64_t *written) {
    fcx_repair_file::Reader F(stdio_read, frep);
    if (F.open()) return say_err(F);
    if (F.kind != '7') { fprintf(stderr, "fcx: repair file: made for the other codec\n"); return -1; }
    const uint32_t B = F.block_bytes;
    std::vector<uint8_t> fillbuf;
    uint64_t n = 0, records = 0;
    bool ok = true, short_seen = false;
    auto bad = [&](uint32_t k, const char *why) {
        fprintf(stderr, "fcx: repair: record %u %s\n", k, why);
        return ok = false;
    };
    const int r = host_each_record(fin, nblocks, [&](uint32_t k, uint32_t, const uint8_t *plain, uint64_t dlen) {
        if (short_seen) return bad(k - 1, "gives a block shorter than the block size and is not the last");
        fcx_repair_entry e;
        const uint8_t *raw = nullptr;
        uint64_t blen;
        const int g = host_entry(&F, k, dlen, &e, &raw, &blen);
        if (g == -2) return bad(k, "decodes to fewer bytes than its entry keeps");
        if (g < 0) return ok = false;
        if (blen == 0 || blen > B) return bad(k, "does not decode to its block's length and has no entry that mends it");
        if (blen < B) short_seen = true;
        const uint64_t keep = g ? e.from : dlen;
        bool w = fwrite(plain, 1, (size_t)keep, fout) == keep;
        if (g && e.len) {
            if (e.kind == FCX_REPAIR_FILL) {
                fillbuf.assign(e.len, (uint8_t)e.fill);
                raw = fillbuf.data();
            }
            w = w && fwrite(raw, 1, e.len, fout) == e.len;
        }
        if (!w) { fprintf(stderr, "write error\n"); return ok = false; }
        n += blen;
        records++;
        return true;
    });
    *written = n;
    if (r || !ok) return -1;
    return F.finish(n, records) ? say_err(F) : 0;
}

// ---- --digest / --test: the printout, the same on the GPU and on the host, and the FCXD file over stdio ----
inline void digest_totals(uint64_t blocks, uint32_t whole) {
    printf("digest: %llu blocks, crc32 %08X\n", (unsigned long long)blocks, whole);
}
// a failing block: its resulting bytes of the block's, its CRC-32 and the digest file's (none: a record
// behind the digest file's last block)
inline void check_line(uint64_t k, uint64_t got, uint64_t blen, uint32_t crc, const uint32_t *expected) {
    printf("block %llu: %llu of %llu bytes, crc32 %08X, expected ", (unsigned long long)k, (unsigned long long)got,
           (unsigned long long)blen, crc);
    if (expected) printf("%08X\n", *expected);
    else printf("none\n");
}
inline void check_extra(uint64_t extra) {
    printf("digest: %llu bytes after the last block\n", (unsigned long long)extra);
}
// the verdict: 0 (OK) when no block fails and the digest file has no block left, else 1 (FAIL)
inline int check_totals(uint64_t bad, uint64_t blocks, uint64_t bytes) {
    const bool ok = bad == 0 && bytes == 0;
    printf("test: %llu of %llu blocks fail, %llu input bytes in them [%s]\n", (unsigned long long)bad,
           (unsigned long long)blocks, (unsigned long long)bytes, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}

// the values of a whole FCXD file (the reader's checks apply), for the expected value a failing block's
// line shows; the file is left at its start.  -1 after a message.
inline int load_digest(FILE *fdig, std::vector<uint32_t> *vals) {
    fcx_digest_file::Reader G(stdio_read, fdig);
    vals->clear();
    if (G.open() || G.take(UINT64_MAX, vals) < 0 || G.finish()) return say_err(G);
    rewind(fdig);
    return 0;
}

// --digest without a device: the FCXD file of forig in blocks of `block` bytes to fdig, the bytes
// fcx_digest_stream writes.  stats: FCX_DIGEST_FILE_STATS values.
inline int host_digest_build(FILE *forig, uint32_t block, FILE *fdig, uint64_t *stats) {
    fcx_digest_file::Writer W(stdio_write, fdig);
    std::vector<uint8_t> buf(block);
    int w = W.begin(block);
    for (size_t got; !w && (got = fread(buf.data(), 1, block, forig)) > 0;) w = W.add(fcx_crc::crc32(0, buf.data(), got), got);
    if (!w && ferror(forig)) { fprintf(stderr, "read error\n"); return -1; }
    if (!w) w = W.finish();
    if (w) return say_err(W);
    const uint64_t s[FCX_DIGEST_FILE_STATS] = {W.n, W.blocks, W.whole};
    if (stats) memcpy(stats, s, sizeof(s));
    return 0;
}

// --test / --digest of a decompress without a device: every FCX7 record through the host decoder, its
// entry of frep (may be null) applied in the sum only, against the FCXD file fdig; the checks and the
// lines of fcx_check_stream.  Returns the verdict (0 / 1), or -1 after a message.
inline int host_check(FILE *fin, FILE *frep, FILE *fdig, uint16_t nblocks, uint64_t *stats) {
    fcx_digest_file::Reader G(stdio_read, fdig);
    if (G.open()) return say_err(G);
    const uint64_t B = G.block_bytes;
    fcx_repair_file::Reader F(stdio_read, frep);
    if (frep) {
        if (F.open()) return say_err(F);
        if (F.kind != '7') { fprintf(stderr, "fcx: repair file: made for the other codec\n"); return -1; }
        if (F.block_bytes != B) { fprintf(stderr, "fcx: repair file: made for another block size than the digest file's\n"); return -1; }
    }
    uint64_t s[6] = {0, 0, UINT64_MAX, 0, 0, 0}, result_bytes = 0;
    bool ok = true;
    std::vector<uint32_t> want;
    const int r = host_each_record(fin, nblocks, [&](uint32_t k, uint32_t, const uint8_t *plain, uint64_t dlen) {
        want.clear();
        const int64_t got = G.take(1, &want);
        const int m = got < 0 ? (int)got : G.more();
        if (m < 0) return ok = say_err(G) == 0;
        const uint64_t blen = got ? (m ? B : G.block_len(k)) : 0;
        fcx_repair_entry e;
        const uint8_t *raw = nullptr;
        uint64_t rlen;
        const int g = host_entry(frep ? &F : nullptr, k, dlen, &e, &raw, &rlen);
        if (g == -2 || (g > 0 && rlen != blen)) fprintf(stderr, "fcx: repair: the entry of record %u does not fit its record\n", k);
        if (g < 0 || (g > 0 && rlen != blen)) return ok = false;
        uint32_t c;
        if (g) {
            c = fcx_crc::crc32(0, plain, e.from);
            c = e.kind == FCX_REPAIR_RAW ? fcx_crc::crc32(c, raw, e.len)
                                         : fcx_crc::combine(c, fcx_crc::crc32_fill((uint8_t)e.fill, e.len), e.len);
        } else {
            c = fcx_crc::crc32(0, plain, dlen);
        }
        s[0]++;
        s[3] += rlen != blen;
        s[5] += dlen;
        result_bytes += rlen;
        if (!got || rlen != blen || c != want[0]) {
            check_line(k, rlen, blen, c, got ? &want[0] : nullptr);
            if (s[1]++ == 0) s[2] = k;
            s[4] += blen;
        }
        return true;
    });
    if (r || !ok) return -1;
    if (frep && F.finish(result_bytes, s[0])) return say_err(F);
    const int64_t left = G.take(UINT64_MAX, nullptr);
    if (left < 0 || G.finish()) return say_err(G);
    if (left) {
        const uint64_t extra = G.n - std::min(G.n, s[0] * B);
        check_extra(extra);
        s[4] += extra;
    }
    if (stats) memcpy(stats, s, sizeof(s));
    return check_totals(s[1], s[0], s[4]);
}

// ---- --find / --find-hex: the printout, the same on the GPU and on the host ----
inline void find_line(uint64_t off) { printf("find: offset %llu\n", (unsigned long long)off); }
inline int find_totals(uint64_t hits, uint64_t decoded) {
    printf("find: %llu hits, decoded bytes = %llu\n", (unsigned long long)hits, (unsigned long long)decoded);
    return 0;
}
// an even number of hex digits, 1 to FCX_FIND_MAX_PATTERN bytes of them; false for anything else
inline bool parse_hex(const char *s, std::vector<uint8_t> *out) {
    out->clear();
    auto nib = [](char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; };
    for (; s[0]; s += 2) {
        const int hi = nib(s[0]), lo = s[1] ? nib(s[1]) : -1;
        if (hi < 0 || lo < 0) return false;
        out->push_back((uint8_t)(16 * hi + lo));
    }
    return !out->empty() && out->size() <= FCX_FIND_MAX_PATTERN;
}

// --find without a device: every FCX7 record through the host decoder, searched behind a rolling tail of
// the last m - 1 decoded bytes, so a match may lie across any number of records; one line per hit unless
// count_only, then the totals.  stats (2 values, may be null): hits, decoded bytes.
inline int host_find(FILE *fin, uint16_t nblocks, const uint8_t *pat, uint32_t m, bool count_only, uint64_t *stats) {
    std::vector<uint8_t> win;   // [tail | record]
    uint64_t pos = 0, hits = 0, tail = 0;   // decoded bytes before the record, hits, bytes of win kept from before
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        win.resize(tail);
        win.insert(win.end(), plain, plain + n);
        const uint64_t len = win.size(), first = pos - tail;   // win[0] is decoded byte `first`
        for (uint64_t p = 0; p + m <= len; p++) {
            const uint8_t *at = (const uint8_t *)memchr(win.data() + p, pat[0], (size_t)(len - m + 1 - p));
            if (!at) break;
            p = (uint64_t)(at - win.data());
            if (memcmp(at, pat, m) == 0) {
                if (!count_only) find_line(first + p);
                hits++;
            }
        }
        pos += n;
        tail = len < m - 1 ? len : m - 1;
        win.erase(win.begin(), win.end() - (ptrdiff_t)tail);
        return true;
    });
    if (r) return r;
    if (stats) {
        stats[0] = hits;
        stats[1] = pos;
    }
    return find_totals(hits, pos);
}

// ---- --count-lines / --lines / --find --line-numbers: the parsers and the printout, the same on the GPU and on the host ----
// "A:N" or "A:" (to the end), A >= 1 the first line as sed counts them: *first 0-based, *count UINT64_MAX for
// "to the end"; false for anything else
inline bool parse_lines(const char *s, uint64_t *first, uint64_t *count) {
    uint64_t v[2] = {0, UINT64_MAX};
    for (int i = 0; i < 2; i++) {
        if (i == 1 && *s == '\0') break;   // "A:"
        if (*s < '0' || *s > '9') return false;
        uint64_t x = 0;
        for (; *s >= '0' && *s <= '9'; s++) {
            if (x > (UINT64_MAX - (uint64_t)(*s - '0')) / 10) return false;
            x = 10 * x + (uint64_t)(*s - '0');
        }
        v[i] = x;
        if (*s != (i == 0 ? ':' : '\0')) return false;
        if (i == 0) s++;
    }
    if (v[0] == 0) return false;
    *first = v[0] - 1;
    *count = v[1];
    return true;
}
// exactly two hex digits
inline bool parse_delim(const char *s, uint8_t *delim) {
    std::vector<uint8_t> one;
    if (strlen(s) != 2 || !parse_hex(s, &one)) return false;
    *delim = one[0];
    return true;
}
inline int lines_totals(uint64_t lines, uint64_t delims, uint64_t decoded) {
    printf("lines: %llu lines, %llu delimiters, decoded bytes = %llu\n", (unsigned long long)lines, (unsigned long long)delims,
           (unsigned long long)decoded);
    return 0;
}
inline int lines_done(uint64_t n, uint64_t off) {
    printf("lines decompress bytes = %llu (offset %llu)\n", (unsigned long long)n, (unsigned long long)off);
    return 0;
}
inline void find_line_numbered(uint64_t off, uint64_t line0) {   // line0: 0-based, printed as sed counts
    printf("find: offset %llu line %llu\n", (unsigned long long)off, (unsigned long long)(line0 + 1));
}

// --count-lines (fout null) and --lines without a device: every FCX7 record through the host decoder, the
// delimiters counted across the records; with fout the bytes of lines [first, first + count) are written and
// the records behind them are not read.  stats (may be null): delimiters, lines, decoded bytes, bytes behind
// the last delimiter (--count-lines); bytes written, their offset (--lines).
inline int host_lines(FILE *fin, uint16_t nblocks, uint8_t delim, FILE *fout, uint64_t first, uint64_t count, uint64_t *stats) {
    const uint64_t end = count < UINT64_MAX - first ? first + count : UINT64_MAX;
    uint64_t pos = 0, nl = 0, last = 0, out = 0, out_off = first == 0 ? 0 : UINT64_MAX;   // out_off: where line `first` starts, once known
    bool io_ok = true;
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        for (uint64_t p = 0; p < n;) {   // [p, q): the rest of line nl inside this record
            const uint8_t *at = (const uint8_t *)memchr(plain + p, delim, (size_t)(n - p));
            const uint64_t q = at ? (uint64_t)(at - plain) + 1 : n;
            if (fout && nl >= first && nl < end) {
                io_ok = io_ok && fwrite(plain + p, 1, (size_t)(q - p), fout) == q - p;
                out += q - p;
            }
            if (at) {
                nl++;
                last = pos + q;
                if (nl == first) out_off = last;
            }
            p = q;
        }
        pos += n;
        return io_ok && !(fout && nl >= end);
    });
    if (r) return r;
    if (!io_ok) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    if (fout) {
        if (out_off == UINT64_MAX) out_off = pos;   // the file has no line `first`: an empty range at its end
        if (stats) {
            stats[0] = out;
            stats[1] = out_off;
        }
        return lines_done(out, out_off);
    }
    const uint64_t s[4] = {nl, nl + (pos > 0 && last != pos), pos, pos - last};
    if (stats) memcpy(stats, s, sizeof(s));
    return lines_totals(s[1], s[0], s[2]);
}

// --find --line-numbers without a device: host_find's walk with the delimiters counted alongside, so every hit
// is printed with the line it lies on.  stats (2 values, may be null): hits, decoded bytes.
inline int host_find_numbered(FILE *fin, uint16_t nblocks, const uint8_t *pat, uint32_t m, uint8_t delim, uint64_t *stats) {
    std::vector<uint8_t> win;   // [tail | record]
    uint64_t pos = 0, hits = 0, tail = 0, nl_first = 0;   // nl_first: delimiters in front of win[0]
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        win.resize(tail);
        win.insert(win.end(), plain, plain + n);
        const uint64_t len = win.size(), first = pos - tail;   // win[0] is decoded byte `first`
        uint64_t seen = 0, nl = nl_first;                      // nl: delimiters in front of win[seen]
        auto advance = [&](uint64_t to) {
            for (; seen < to; seen++) nl += win[seen] == delim;
        };
        for (uint64_t p = 0; p + m <= len; p++) {
            const uint8_t *at = (const uint8_t *)memchr(win.data() + p, pat[0], (size_t)(len - m + 1 - p));
            if (!at) break;
            p = (uint64_t)(at - win.data());
            if (memcmp(at, pat, m) == 0) {
                advance(p);
                find_line_numbered(first + p, nl);
                hits++;
            }
        }
        pos += n;
        tail = len < m - 1 ? len : m - 1;
        advance(len - tail);
        nl_first = nl;
        win.erase(win.begin(), win.end() - (ptrdiff_t)tail);
        return true;
    });
    if (r) return r;
    if (stats) {
        stats[0] = hits;
        stats[1] = pos;
    }
    return find_totals(hits, pos);
}

// ---- --cut-fields / --cut-bytes: the printout, the same on the GPU and on the host ----
// stats: the FCX_CUT_STATS values
inline int cut_totals(const uint64_t *stats) {
    printf("cut: %llu bytes, %llu delimiters, %llu separators (%llu kept), decoded bytes = %llu\n", (unsigned long long)stats[0],
           (unsigned long long)stats[2], (unsigned long long)stats[3], (unsigned long long)stats[4], (unsigned long long)stats[1]);
    return 0;
}

// The cut without a device: every FCX7 record through the host decoder and the rule of fcx_cut.h, the open line's tick
// count carried across the records; the kept bytes to fout (null: --count).  stats (FCX_CUT_STATS values, may be null;
// groups: the records).
inline int host_cut(FILE *fin, uint16_t nblocks, const fcx_cut &cut, FILE *fout, uint64_t *stats) {
    uint64_t s[FCX_CUT_STATS] = {};
    uint32_t ticks = 0;
    bool io_ok = true;
    std::string kept;
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        kept.clear();
        fcx::cut_host_bytes(cut, plain, n, &ticks, fout ? &kept : nullptr, s);
        s[5]++;
        if (fout && !kept.empty()) io_ok = fwrite(kept.data(), 1, kept.size(), fout) == kept.size();
        return io_ok;
    });
    if (r) return r;
    if (!io_ok) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    if (stats) memcpy(stats, s, sizeof(s));
    return cut_totals(s);
}

// ---- --grep / --grep-hex: the printout, the same on the GPU and on the host ----
inline int grep_totals(uint64_t lines, uint64_t bytes, uint64_t hits, uint64_t decoded) {
    printf("grep: %llu lines, %llu bytes, %llu hits, decoded bytes = %llu\n", (unsigned long long)lines, (unsigned long long)bytes,
           (unsigned long long)hits, (unsigned long long)decoded);
    return 0;
}
// does the pattern hold the delimiter?  (then no line can hold the pattern: a usage error)
inline bool pattern_holds(const std::vector<uint8_t> &pat, uint8_t delim) { return memchr(pat.data(), delim, pat.size()) != nullptr; }

// --grep without a device: every FCX7 record through the host decoder, cut into lines across the records; the
// open line is buffered (a hit lies wholly inside a line, so a line is searched once, when it closes or the
// file ends) and written to fout (null: --count) when it holds the pattern.  stats (4 values, may be null):
// lines, bytes, hits, decoded bytes.
inline int host_grep(FILE *fin, uint16_t nblocks, uint8_t delim, const uint8_t *pat, uint32_t m, FILE *fout, uint64_t *stats) {
    std::vector<uint8_t> line;   // the open line so far
    uint64_t pos = 0, lines = 0, bytes = 0, hits = 0;
    bool failed = false;
    auto close_line = [&]() {
        uint64_t h = 0;
        const uint64_t len = line.size();
        for (uint64_t p = 0; p + m <= len; p++) {
            const uint8_t *at = (const uint8_t *)memchr(line.data() + p, pat[0], (size_t)(len - m + 1 - p));
            if (!at) break;
            p = (uint64_t)(at - line.data());
            h += memcmp(at, pat, m) == 0;
        }
        if (h) {
            hits += h;
            lines++;
            bytes += len;
            if (fout && fwrite(line.data(), 1, (size_t)len, fout) != len) failed = true;
        }
        line.clear();
    };
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        for (uint64_t p = 0; p < n;) {
            const uint8_t *at = (const uint8_t *)memchr(plain + p, delim, (size_t)(n - p));
            const uint64_t q = at ? (uint64_t)(at - plain) + 1 : n;   // the line's bytes in this record end here
            line.insert(line.end(), plain + p, plain + q);
            if (at) close_line();
            p = q;
        }
        pos += n;
        return !failed;
    });
    if (r) return r;
    if (!line.empty()) close_line();   // the unterminated tail is a line
    if (failed) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    if (stats) {
        stats[0] = lines;
        stats[1] = bytes;
        stats[2] = hits;
        stats[3] = pos;
    }
    return grep_totals(lines, bytes, hits, pos);
}

// ---- --find-set / --grep-set / --ignore-case: the pattern file, the printout and the host paths ----
inline int find_set_totals(uint64_t hits, uint64_t decoded, uint32_t npat) {
    printf("find: %llu hits, decoded bytes = %llu, patterns: %u\n", (unsigned long long)hits, (unsigned long long)decoded, npat);
    return 0;
}
inline int grep_set_totals(uint64_t lines, uint64_t bytes, uint64_t hits, uint64_t decoded, uint32_t npat) {
    printf("grep: %llu lines, %llu bytes, %llu hits, decoded bytes = %llu, patterns: %u\n", (unsigned long long)lines,
           (unsigned long long)bytes, (unsigned long long)hits, (unsigned long long)decoded, npat);
    return 0;
}

// The patterns of a pattern file's bytes: separated by 0x0A, one trailing 0x0A allowed; hex: every line is an even
// number of hex digits.  bytes: their concatenation, lens: their lengths.  False for an empty pattern (grep -f
// would match every line there), more than FCX_SET_MAX_PATTERNS patterns, a pattern of more than
// FCX_FIND_MAX_PATTERN bytes, more than FCX_SET_MAX_BYTES in all, bad hex, or no pattern at all.
inline bool parse_patterns(const uint8_t *text, uint64_t n, bool hex, std::vector<uint8_t> *bytes, std::vector<uint32_t> *lens) {
    bytes->clear();
    lens->clear();
    if (n && text[n - 1] == 0x0A) n--;
    if (n == 0) return false;
    for (uint64_t p = 0; p <= n;) {
        const uint8_t *at = p < n ? (const uint8_t *)memchr(text + p, 0x0A, (size_t)(n - p)) : nullptr;
        const uint64_t q = at ? (uint64_t)(at - text) : n;
        std::vector<uint8_t> pat(text + p, text + q);
        if (hex) {
            const std::string digits(pat.begin(), pat.end());
            if (digits.find('\0') != std::string::npos || !parse_hex(digits.c_str(), &pat)) return false;
        }
        if (pat.empty() || pat.size() > FCX_FIND_MAX_PATTERN || lens->size() == FCX_SET_MAX_PATTERNS) return false;
        bytes->insert(bytes->end(), pat.begin(), pat.end());
        lens->push_back((uint32_t)pat.size());
        if (bytes->size() > FCX_SET_MAX_BYTES) return false;
        p = q + 1;
    }
    return true;
}
inline bool load_patterns(const char *path, bool hex, std::vector<uint8_t> *bytes, std::vector<uint32_t> *lens) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::vector<uint8_t> text;
    uint8_t buf[4096];
    for (size_t g; (g = fread(buf, 1, sizeof(buf), f)) > 0 && text.size() <= 4 * FCX_SET_MAX_BYTES + 4096;) text.insert(text.end(), buf, buf + g);
    fclose(f);
    return parse_patterns(text.data(), text.size(), hex, bytes, lens);
}

// the patterns of the set that occur at win[p] and end at or in front of `end`: bit k per pattern (win: folded bytes)
inline uint64_t set_occurs(const fcx_pattern_set &S, const uint8_t *win, uint64_t p, uint64_t end) {
    uint64_t mk = ((const uint64_t *)(S.block + fcx::kPsT0))[win[p]], got = 0;
    for (; mk; mk &= mk - 1) {
        const uint32_t k = (uint32_t)__builtin_ctzll(mk);
        if (p + S.len[k] <= end && memcmp(win + p, S.pat(k), S.len[k]) == 0) got |= 1ull << k;
    }
    return got;
}

// --find-set without a device: every FCX7 record through the host decoder, folded when the set folds, searched
// behind a rolling tail of the last M - 1 decoded bytes (M the longest pattern): a record's scan judges the
// positions every pattern fits behind, the file's end the rest with each pattern bounded by it.  One line per hit
// unless count_only, then the totals.  stats (2 values, may be null): hits, decoded bytes; counts (may be null):
// per pattern the positions at which it occurs.
inline int host_find_set(FILE *fin, uint16_t nblocks, const fcx_pattern_set &S, bool count_only, uint64_t *stats, uint64_t *counts) {
    std::vector<uint8_t> win;   // [tail | record], folded
    std::vector<uint64_t> per(S.npat, 0);
    uint64_t pos = 0, hits = 0, tail = 0;
    const uint64_t M = S.max_len;
    auto judge = [&](uint64_t p0, uint64_t p1, uint64_t first) {
        for (uint64_t p = p0; p < p1; p++) {
            const uint64_t got = set_occurs(S, win.data(), p, win.size());
            if (!got) continue;
            for (uint64_t g = got; g; g &= g - 1) per[__builtin_ctzll(g)]++;
            if (!count_only) find_line(first + p);
            hits++;
        }
    };
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        win.resize(tail);
        for (uint64_t i = 0; i < n; i++) win.push_back(S.fold(plain[i]));
        const uint64_t len = win.size();
        judge(0, len >= M ? len - M + 1 : 0, pos - tail);
        pos += n;
        tail = len < M - 1 ? len : M - 1;
        win.erase(win.begin(), win.end() - (ptrdiff_t)tail);
        return true;
    });
    if (r) return r;
    judge(0, win.size(), pos - win.size());   // the positions the last record carried, each pattern bounded by the end
    if (stats) {
        stats[0] = hits;
        stats[1] = pos;
    }
    for (uint32_t k = 0; k < S.npat && counts; k++) counts[k] = per[k];
    return find_set_totals(hits, pos, S.npat);
}

// --grep-set without a device: host_grep with a set: the open line is buffered, raw for the output and folded for
// the search; a line is searched once, when it closes or the file ends.  stats (4 values, may be null): lines,
// bytes, hits, decoded bytes; counts as host_find_set's.
inline int host_grep_set(FILE *fin, uint16_t nblocks, uint8_t delim, const fcx_pattern_set &S, FILE *fout, uint64_t *stats,
                         uint64_t *counts) {
    std::vector<uint8_t> line, folded;   // the open line so far
    std::vector<uint64_t> per(S.npat, 0);
    uint64_t pos = 0, lines = 0, bytes = 0, hits = 0;
    bool failed = false;
    auto close_line = [&]() {
        uint64_t h = 0;
        const uint64_t len = line.size();
        folded.resize(len);
        for (uint64_t i = 0; i < len; i++) folded[i] = S.fold(line[i]);
        for (uint64_t p = 0; p < len; p++) {
            const uint64_t got = set_occurs(S, folded.data(), p, len);
            for (uint64_t g = got; g; g &= g - 1) per[__builtin_ctzll(g)]++;
            h += got != 0;
        }
        if (h) {
            hits += h;
            lines++;
            bytes += len;
            if (fout && fwrite(line.data(), 1, (size_t)len, fout) != len) failed = true;
        }
        line.clear();
    };
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        for (uint64_t p = 0; p < n;) {
            const uint8_t *at = (const uint8_t *)memchr(plain + p, delim, (size_t)(n - p));
            const uint64_t q = at ? (uint64_t)(at - plain) + 1 : n;   // the line's bytes in this record end here
            line.insert(line.end(), plain + p, plain + q);
            if (at) close_line();
            p = q;
        }
        pos += n;
        return !failed;
    });
    if (r) return r;
    if (!line.empty()) close_line();   // the unterminated tail is a line
    if (failed) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    if (stats) {
        stats[0] = lines;
        stats[1] = bytes;
        stats[2] = hits;
        stats[3] = pos;
    }
    for (uint32_t k = 0; k < S.npat && counts; k++) counts[k] = per[k];
    return grep_set_totals(lines, bytes, hits, pos, S.npat);
}

// ---- --invert / --before / --after / --context: the value parser, the printout and the host path ----
// a count of context lines: decimal digits alone, at most FCX_GREP_MAX_CONTEXT
inline bool parse_context(const char *s, uint32_t *n) {
    const size_t len = strlen(s);
    if (len < 1 || len > 9 || strspn(s, "0123456789") != len) return false;
    const unsigned long v = strtoul(s, nullptr, 10);
    if (v > FCX_GREP_MAX_CONTEXT) return false;
    *n = (uint32_t)v;
    return true;
}
inline int grep_blocks_totals(uint64_t blocks, uint64_t lines, uint64_t base, uint64_t bytes, uint64_t hits, uint64_t decoded) {
    printf("grep: %llu blocks, %llu lines, %llu base lines, %llu bytes, %llu hits, decoded bytes = %llu\n", (unsigned long long)blocks,
           (unsigned long long)lines, (unsigned long long)base, (unsigned long long)bytes, (unsigned long long)hits,
           (unsigned long long)decoded);
    return 0;
}
// the line GNU grep prints between two blocks when a context was asked for
inline const char *block_separator(const fcx_grep_opts &o) { return o.before || o.after ? "--\n" : ""; }

// The context grep without a device: host_grep_set's lines, each judged when it closes.  A base line (it holds a
// pattern, or with FCX_GREP_INVERT holds none) is written behind the lines waiting in front of it and opens an
// after-context of opts.after lines; a line that is neither waits, the last opts.before of them at most.  A line
// written behind a line that was dropped starts a block: block_separator() goes in front of every block but the first.
// stats (6 values, may be null): blocks, lines, base lines, bytes, hits, decoded bytes; counts as host_find_set's.
// separators false: no line between blocks (a caller that cuts the blocks' bytes: the `--` line is not a byte of the file).
inline int host_grep_blocks(FILE *fin, uint16_t nblocks, uint8_t delim, const fcx_pattern_set &S, const fcx_grep_opts &opts, FILE *fout,
                            uint64_t *stats, uint64_t *counts, bool separators = true) {
    std::vector<uint8_t> line, folded;       // the open line so far
    std::vector<std::vector<uint8_t>> wait;  // the unselected lines right in front of the open one, opts.before at most
    std::vector<uint64_t> per(S.npat, 0);
    const std::string sep = separators ? block_separator(opts) : "";
    const bool invert = (opts.flags & FCX_GREP_INVERT) != 0;
    uint64_t pos = 0, blocks = 0, lines = 0, base = 0, bytes = 0, hits = 0, after_left = 0;
    uint64_t dropped = 0;   // lines since the last written one that no longer wait: a line written behind them starts a block
    bool failed = false;
    auto put = [&](const std::vector<uint8_t> &l) {
        if (lines == 0 || dropped) {
            if (blocks && fout && !sep.empty() && fwrite(sep.data(), 1, sep.size(), fout) != sep.size()) failed = true;
            blocks++;
        }
        dropped = 0;
        lines++;
        bytes += l.size();
        if (fout && fwrite(l.data(), 1, l.size(), fout) != l.size()) failed = true;
    };
    auto close_line = [&]() {
        uint64_t h = 0;
        const uint64_t len = line.size();
        folded.resize(len);
        for (uint64_t i = 0; i < len; i++) folded[i] = S.fold(line[i]);
        for (uint64_t p = 0; p < len; p++) {
            const uint64_t got = set_occurs(S, folded.data(), p, len);
            for (uint64_t g = got; g; g &= g - 1) per[__builtin_ctzll(g)]++;
            h += got != 0;
        }
        hits += h;
        if ((h != 0) != invert) {
            base++;
            for (const std::vector<uint8_t> &w : wait) put(w);
            wait.clear();
            put(line);
            after_left = opts.after;
        } else if (after_left) {
            put(line);
            after_left--;
        } else if (opts.before == 0) {
            dropped++;
        } else {
            if (wait.size() == opts.before) {
                wait.erase(wait.begin());
                dropped++;
            }
            wait.push_back(line);
        }
        line.clear();
    };
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        for (uint64_t p = 0; p < n;) {
            const uint8_t *at = (const uint8_t *)memchr(plain + p, delim, (size_t)(n - p));
            const uint64_t q = at ? (uint64_t)(at - plain) + 1 : n;   // the line's bytes in this record end here
            line.insert(line.end(), plain + p, plain + q);
            if (at) close_line();
            p = q;
        }
        pos += n;
        return !failed;
    });
    if (r) return r;
    if (!line.empty()) close_line();   // the unterminated tail is a line
    if (failed) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    if (stats) {
        stats[0] = blocks;
        stats[1] = lines;
        stats[2] = base;
        stats[3] = bytes;
        stats[4] = hits;
        stats[5] = pos;
    }
    for (uint32_t k = 0; k < S.npat && counts; k++) counts[k] = per[k];
    return grep_blocks_totals(blocks, lines, base, bytes, hits, pos);
}

// ---- --grep-regex: the host path ----
// The regex grep without a device: host_grep_blocks with the compiled table (fcx_regex.h) run byte by byte over every
// closed line in the place of the set's compare; the delimiter is the regex's.  A position is a hit when the state
// behind its byte is in acc, or in acc_eol with the delimiter or the line's end behind it.  `blocks`: the options were
// given, so the totals are the context grep's (and block_separator() goes between blocks); otherwise the set grep's
// with one pattern.  stats (6 values, may be null): blocks, lines, base lines, bytes, hits, decoded bytes.  separators: as
// host_grep_blocks'.
inline int host_grep_regex(FILE *fin, uint16_t nblocks, const fcx_regex &R, const fcx_grep_opts &opts, bool blocks_form, FILE *fout,
                           uint64_t *stats, bool separators = true) {
    std::vector<uint8_t> line;               // the open line so far
    std::vector<std::vector<uint8_t>> wait;  // the unselected lines right in front of the open one, opts.before at most
    const std::string sep = separators ? block_separator(opts) : "";
    const bool invert = (opts.flags & FCX_GREP_INVERT) != 0;
    const uint8_t delim = R.delim;
    uint64_t pos = 0, blocks = 0, lines = 0, base = 0, bytes = 0, hits = 0, after_left = 0;
    uint64_t dropped = 0;   // lines since the last written one that no longer wait: a line written behind them starts a block
    bool failed = false;
    auto put = [&](const std::vector<uint8_t> &l) {
        if (lines == 0 || dropped) {
            if (blocks && fout && !sep.empty() && fwrite(sep.data(), 1, sep.size(), fout) != sep.size()) failed = true;
            blocks++;
        }
        dropped = 0;
        lines++;
        bytes += l.size();
        if (fout && fwrite(l.data(), 1, l.size(), fout) != l.size()) failed = true;
    };
    auto close_line = [&]() {
        uint64_t h = 0;
        const uint64_t len = line.size(), body = len && line[len - 1] == delim ? len - 1 : len;
        uint8_t st = (uint8_t)R.start;
        for (uint64_t p = 0; p < body; p++) {
            st = R.step(st, line[p]);
            h += R.hit(st, p + 1 == body);
        }
        hits += h;
        if ((h != 0) != invert) {
            base++;
            for (const std::vector<uint8_t> &w : wait) put(w);
            wait.clear();
            put(line);
            after_left = opts.after;
        } else if (after_left) {
            put(line);
            after_left--;
        } else if (opts.before == 0) {
            dropped++;
        } else {
            if (wait.size() == opts.before) {
                wait.erase(wait.begin());
                dropped++;
            }
            wait.push_back(line);
        }
        line.clear();
    };
    const int r = host_each_record(fin, nblocks, [&](uint32_t, uint32_t, const uint8_t *plain, uint64_t n) {
        for (uint64_t p = 0; p < n;) {
            const uint8_t *at = (const uint8_t *)memchr(plain + p, delim, (size_t)(n - p));
            const uint64_t q = at ? (uint64_t)(at - plain) + 1 : n;   // the line's bytes in this record end here
            line.insert(line.end(), plain + p, plain + q);
            if (at) close_line();
            p = q;
        }
        pos += n;
        return !failed;
    });
    if (r) return r;
    if (!line.empty()) close_line();   // the unterminated tail is a line
    if (failed) {
        fprintf(stderr, "write error\n");
        return -1;
    }
    if (stats) {
        stats[0] = blocks;
        stats[1] = lines;
        stats[2] = base;
        stats[3] = bytes;
        stats[4] = hits;
        stats[5] = pos;
    }
    return blocks_form ? grep_blocks_totals(blocks, lines, base, bytes, hits, pos) : grep_set_totals(lines, bytes, hits, pos, 1);
}

}  // namespace fcx_cli


#endif  // FCX_CLI_HOST_H
