// fcx_digest_file.h — the FCXD file (include/fcx.h): its canonical writer and its
// streaming reader, over the read / write callbacks of the stream paths.  Host code only, shared by the
// library's stream forms (fcx_stream.hip) and the command line's no-device path
// (fcx_cli_host.h), so both write the same bytes and reject the same files.
#ifndef FCX_DIGEST_FILE_H
#define FCX_DIGEST_FILE_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "fcx.h"
#include "fcx_crc32.h"
#include "fcx_sidecar_io.h"

namespace fcx_digest_file {

using namespace fcx_sidecar;

constexpr uint32_t kSection = FCX_DIGEST_SECTION;   // values of a section at most; the writer's: exactly, but the last

// Canonical writer.  add() takes the blocks' CRC-32 and lengths in block order; a section is written
// when it holds kSection values, or at finish().  Every function returns 0, or a negative code with the
// reason in `err`.
struct Writer : WriteBase {
    std::vector<uint8_t> sec;   // the values of the section in hand, as written
    uint64_t n = 0, blocks = 0;
    uint32_t whole = 0, self = 0;   // the CRC-32 of the bytes so far, of the values so far

    using WriteBase::WriteBase;
    int begin(uint32_t block_bytes) {
        uint8_t h[FCX_DIGEST_HEADER_BYTES] = {'F', 'C', 'X', 'D', 1, 0, 0, 0};
        put32(h + 8, block_bytes);
        put32(h + 12, 0);
        return put(h, sizeof(h));
    }
    int flush() {
        if (sec.empty()) return 0;
        uint8_t h[8];
        put32(h, (uint32_t)(sec.size() / 4));
        put32(h + 4, 0);
        int r = put(h, sizeof(h));
        if (!r) r = put(sec.data(), sec.size());
        sec.clear();
        return r;
    }
    int add(uint32_t crc, uint64_t len) {
        uint8_t v[4];
        put32(v, crc);
        sec.insert(sec.end(), v, v + 4);
        self = fcx_crc::crc32(self, v, 4);
        whole = fcx_crc::combine(whole, crc, len);
        n += len;
        blocks++;
        return sec.size() == 4ull * kSection ? flush() : 0;
    }
    int finish() {
        int r = flush();
        if (r) return r;
        uint8_t t[8 + FCX_DIGEST_TRAILER_BYTES] = {};   // the count of 0 that ends the sections, then the trailer
        put64(t + 8, n);
        put64(t + 16, blocks);
        put32(t + 24, whole);
        put32(t + 28, self);
        return put(t, sizeof(t));
    }
};

// Streaming reader: open() takes the header; take(want, out) appends the next values, fewer than `want`
// only when the sections end; more() says whether a value is left, reading a further section when the one
// in memory is used up, and once the sections end it reads the trailer and checks it against what was
// read; finish() expects the end of the file.  One section is in memory at a time.  The block lengths
// follow from the trailer's n: every block holds block_bytes but the last.  Returns as noted, or
// FCX_ERR_FORMAT (or the read callback's error) with the reason in `err`.
struct Reader : ReadBase {
    uint32_t block_bytes = 0;
    std::vector<uint32_t> sec;
    size_t cur = 0;
    bool at_trailer = false, held = false;
    uint64_t n = 0, blocks = 0, seen = 0;
    uint32_t whole = 0, self = 0, acc = 0, last = 0;   // (acc: the CRC-32 of the blocks before `last`)

    Reader(fcx_read_fn r, void *u) : ReadBase("digest file: ", r, u) {}
    int open() {
        uint8_t h[FCX_DIGEST_HEADER_BYTES];
        int r = get(h, sizeof(h));
        if (r) return r;
        if (memcmp(h, "FCXD", 4) != 0) return bad("not an FCXD file");
        if (h[4] != 1) return bad("unknown version");
        if (h[5] || h[6] || h[7] || get32(h + 12)) return bad("bad header");
        block_bytes = get32(h + 8);
        if (block_bytes == 0 || block_bytes > FCX_MAX_BLOCK_BYTES) return bad("block size outside [1, FCX_MAX_BLOCK_BYTES]");
        return 0;
    }
    // the next section, or the end of the sections and the trailer
    int load() {
        uint8_t h[8];
        int r = get(h, sizeof(h));
        if (r) return r;
        sec.clear();
        cur = 0;
        const uint32_t count = get32(h);
        if (get32(h + 4)) return bad("a section's reserved field is not 0");
        if (count > kSection) return bad("a section of more than 4096 values");
        if (count == 0) {
            uint8_t t[FCX_DIGEST_TRAILER_BYTES];
            if ((r = get(t, sizeof(t)))) return r;
            n = get64(t);
            blocks = get64(t + 8);
            whole = get32(t + 16);
            at_trailer = true;
            if (blocks != seen) return bad("the trailer's block count is not the sections'");
            if (get32(t + 20) != self) return bad("the trailer's check of the values fails: a value is damaged");
            if (blocks != (n + block_bytes - 1) / block_bytes) return bad("the trailer's blocks are not ceil(n / block size)");
            const uint32_t all = held ? fcx_crc::combine(acc, last, n - (blocks - 1) * (uint64_t)block_bytes) : 0u;
            if (all != whole) return bad("the trailer's CRC-32 of the whole is not the blocks' combined");
            return 0;
        }
        std::vector<uint8_t> raw(4ull * count);
        if ((r = get(raw.data(), raw.size()))) return r;
        self = fcx_crc::crc32(self, raw.data(), raw.size());
        sec.resize(count);
        for (uint32_t i = 0; i < count; i++) {
            sec[i] = get32(raw.data() + 4 * i);
            if (held) acc = fcx_crc::combine(acc, last, block_bytes);
            last = sec[i];
            held = true;
        }
        seen += count;
        return 0;
    }
    // 1: a value is left; 0: the sections have ended (the trailer is read and holds); < 0: an error
    int more() {
        while (!at_trailer && cur == sec.size()) {
            const int r = load();
            if (r) return r;
        }
        return at_trailer ? 0 : 1;
    }
    // appends up to `want` values to *out (nullptr: drops them); the count, or < 0
    int64_t take(uint64_t want, std::vector<uint32_t> *out) {
        uint64_t got = 0;
        while (got < want) {
            const int m = more();
            if (m < 0) return m;
            if (m == 0) break;
            const uint64_t k = std::min<uint64_t>(want - got, sec.size() - cur);
            if (out) out->insert(out->end(), sec.begin() + cur, sec.begin() + cur + k);
            cur += k;
            got += k;
        }
        return (int64_t)got;
    }
    // after the last value: the trailer (if not read yet), then nothing
    int finish() {
        const int m = more();
        if (m < 0) return m;
        if (m > 0) return bad("values behind the ones that were asked for");
        return expect_end();
    }
    // length of block k of the file (needs the trailer: more() == 0)
    uint64_t block_len(uint64_t k) const {
        const uint64_t o0 = k * (uint64_t)block_bytes;
        return o0 < n ? std::min<uint64_t>(block_bytes, n - o0) : 0;
    }
};

}  // namespace fcx_digest_file

#endif  // FCX_DIGEST_FILE_H
