// fcx_repair_file.h — the FCXR file (include/fcx.h): its canonical writer and its
// on-demand reader, over the read / write callbacks of the stream paths.  Host code only, shared by
// the library's stream forms (fcx_stream.hip) and the command line's no-device path (fcx_cli_host.h),
// so both write the same bytes and reject the same files.
#ifndef FCX_REPAIR_FILE_H
#define FCX_REPAIR_FILE_H

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_sidecar_io.h"

namespace fcx_repair_file {

using namespace fcx_sidecar;

constexpr uint32_t kWindow = 256;          // entries of a section at most; the writer's sections: block >> 8
constexpr uint32_t kTrailerMark = 0xFFFFFFFFu;

// Canonical writer.  add() takes the entries in ascending file-wide block order with their RAW bytes;
// a section is written when an entry of the next window arrives, or at finish().  Every function
// returns 0, or a negative code with the reason in `err`.
struct Writer : WriteBase {
    std::vector<fcx_repair_entry> sec;
    std::vector<uint8_t> data;
    uint64_t entries = 0, data_bytes = 0, last_block = 0;

    using WriteBase::WriteBase;
    int begin(char kind, uint32_t block_bytes) {
        uint8_t h[FCX_REPAIR_HEADER_BYTES] = {'F', 'C', 'X', 'R', 1, (uint8_t)kind, 0, 0};
        put32(h + 8, block_bytes);
        put32(h + 12, 0);
        return put(h, sizeof(h));
    }
    int flush() {
        if (sec.empty()) return 0;
        uint8_t h[16];
        put32(h, (uint32_t)sec.size());
        put32(h + 4, 0);
        put64(h + 8, data.size());
        int r = put(h, sizeof(h));
        if (!r) r = put(sec.data(), sec.size() * sizeof(fcx_repair_entry));
        if (!r) r = put(data.data(), data.size());
        sec.clear();
        data.clear();
        return r;
    }
    int add(fcx_repair_entry e, const uint8_t *raw) {
        if (entries && e.block <= last_block) {
            err = "repair entries do not ascend";
            return FCX_ERR_INTERNAL;
        }
        if (!sec.empty() && (sec.back().block >> 8) != (e.block >> 8)) {
            const int r = flush();
            if (r) return r;
        }
        e.data_off = 0;
        if (e.kind == FCX_REPAIR_RAW) {
            e.data_off = data.size();
            data.insert(data.end(), raw, raw + e.len);
            data_bytes += e.len;
        }
        sec.push_back(e);
        last_block = e.block;
        entries++;
        return 0;
    }
    int finish(uint64_t n, uint64_t records) {
        int r = flush();
        if (r) return r;
        uint8_t t[FCX_REPAIR_TRAILER_BYTES];
        put32(t, kTrailerMark);
        put32(t + 4, 0);
        put64(t + 8, n);
        put64(t + 16, records);
        put64(t + 24, entries);
        put64(t + 32, data_bytes);
        return put(t, sizeof(t));
    }
};

// On-demand reader: open() takes the header; next(limit, ...) hands out the next entry while its block
// is below `limit` (the end of the record group in hand), reading a further section only when the
// one in memory is used up; finish() expects the trailer next and checks it.  One section is in memory
// at a time: <= 256 entries and <= 256 blocks of data.  Blocks must ascend strictly over the whole
// file; where the section boundaries fall does not matter.  Returns as noted, or FCX_ERR_FORMAT (or
// the read callback's error) with the reason in `err`.
struct Reader : ReadBase {
    char kind = 0;
    uint32_t block_bytes = 0;
    std::vector<fcx_repair_entry> sec;
    std::vector<uint8_t> data;
    size_t cur = 0;
    bool at_trailer = false, any = false;
    uint64_t last_block = 0, entries = 0, data_bytes = 0;
    uint8_t trailer[FCX_REPAIR_TRAILER_BYTES];

    Reader(fcx_read_fn r, void *u) : ReadBase("repair file: ", r, u) {}
    int open() {
        uint8_t h[FCX_REPAIR_HEADER_BYTES];
        int r = get(h, sizeof(h));
        if (r) return r;
        if (memcmp(h, "FCXR", 4) != 0) return bad("not an FCXR file");
        if (h[4] != 1) return bad("unknown version");
        if ((h[5] != '7' && h[5] != '8') || h[6] || h[7] || get32(h + 12)) return bad("bad header");
        kind = (char)h[5];
        block_bytes = get32(h + 8);
        if (block_bytes == 0 || block_bytes > FCX_MAX_BLOCK_BYTES) return bad("block size outside [1, FCX_MAX_BLOCK_BYTES]");
        return 0;
    }
    // the next section, or the trailer
    int load() {
        uint8_t h[16];
        int r = get(h, sizeof(h));
        if (r) return r;
        sec.clear();
        data.clear();
        cur = 0;
        const uint32_t ne = get32(h);
        if (ne == kTrailerMark) {
            memcpy(trailer, h, 16);
            if ((r = get(trailer + 16, sizeof(trailer) - 16))) return r;
            at_trailer = true;
            return 0;
        }
        const uint64_t nd = get64(h + 8);
        if (ne == 0 || ne > kWindow || get32(h + 4)) return bad("a section has no entries, or more than 256");
        if (nd > (uint64_t)ne * block_bytes) return bad("a section's data is larger than its blocks");
        sec.resize(ne);
        if ((r = get((uint8_t *)sec.data(), (uint64_t)ne * sizeof(fcx_repair_entry)))) return r;
        data.resize(nd);
        if ((r = get(data.data(), nd))) return r;
        for (const fcx_repair_entry &e : sec) {
            if (any && e.block <= last_block) return bad("blocks do not ascend");
            if (e.kind > FCX_REPAIR_FILL) return bad("unknown entry kind");
            if ((uint64_t)e.from + e.len > block_bytes) return bad("an entry is longer than a block");
            if (e.kind == FCX_REPAIR_RAW && (e.data_off > nd || e.len > nd - e.data_off)) return bad("RAW bytes outside the section's data");
            any = true;
            last_block = e.block;
        }
        return 0;
    }
    // 1: *e (block file-wide) and *raw (its RAW bytes, valid until the next call) are the next entry, whose
    // block is in [first, limit); 0: the next entry, if any, is at or past limit; < 0: an error
    int next(uint64_t first, uint64_t limit, fcx_repair_entry *e, const uint8_t **raw) {
        while (!at_trailer && cur == sec.size()) {
            const int r = load();
            if (r) return r;
        }
        if (at_trailer || sec[cur].block >= limit) return 0;
        if (sec[cur].block < first) return bad("an entry for a block that is already written");
        *e = sec[cur++];
        *raw = e->kind == FCX_REPAIR_RAW ? data.data() + e->data_off : nullptr;
        entries++;
        if (e->kind == FCX_REPAIR_RAW) data_bytes += e->len;
        return 1;
    }
    // after the last record: nothing but the trailer may follow, and it must say what was seen
    int finish(uint64_t n, uint64_t records) {
        fcx_repair_entry e;
        const uint8_t *raw;
        const int r = next(records, ~0ull, &e, &raw);
        if (r < 0) return r;
        if (r > 0) return bad("an entry for a block behind the last record");
        if (get32(trailer + 4)) return bad("bad trailer");
        if (get64(trailer + 16) != records) return bad("the trailer's record count is not the file's");
        if (get64(trailer + 8) != n) return bad("the trailer's byte count is not what was written");
        if (get64(trailer + 24) != entries || get64(trailer + 32) != data_bytes) return bad("the trailer's entry counts are not the sections'");
        return expect_end();
    }
};

// is [p, p + len) one byte value?  (len <= 1: yes)
inline bool one_value(const uint8_t *p, uint64_t len) {
    for (uint64_t i = 1; i < len; i++)
        if (p[i] != p[0]) return false;
    return true;
}

// the entry of record `block` from its decoded bytes and its block of the original, as include/fcx.h
// defines it; false when the record comes back (no entry)
inline bool plan_entry(uint64_t block, const uint8_t *dec, uint64_t dlen, const uint8_t *orig, uint64_t blen,
                       fcx_repair_entry *e) {
    const uint64_t m = dlen < blen ? dlen : blen;
    uint64_t fd = 0;
    while (fd < m && dec[fd] == orig[fd]) fd++;
    if (fd == m && dlen == blen) return false;
    const uint64_t len = blen - fd;
    const bool fill = one_value(orig + fd, len);
    e->block = block;
    e->data_off = 0;
    e->from = (uint32_t)fd;
    e->len = (uint32_t)len;
    e->kind = fill ? FCX_REPAIR_FILL : FCX_REPAIR_RAW;
    e->fill = fill && len ? orig[fd] : 0;
    return true;
}

}  // namespace fcx_repair_file

#endif  // FCX_REPAIR_FILE_H
