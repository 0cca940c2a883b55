// fcx_sidecar_io.h — the byte-level plumbing the two sidecar files share (fcx_repair_file.h, FCXR;
// fcx_digest_file.h, FCXD): little-endian fields, a write side that turns a failing write callback
// into `err`, and a read side that takes exactly n bytes or says "truncated".  Host code only; the
// layouts and their checks stay with each file.
#ifndef FCX_SIDECAR_IO_H
#define FCX_SIDECAR_IO_H

#include <cstdint>
#include <cstring>
#include <string>

#include "fcx.h"

namespace fcx_sidecar {

inline void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
inline uint32_t get32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t get64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }

// Every function returns 0, or a negative code with the reason in `err`.
struct WriteBase {
    fcx_write_fn wr;
    void *user;
    std::string err;

    WriteBase(fcx_write_fn w, void *u) : wr(w), user(u) {}
    int put(const void *p, uint64_t n) {
        if (n == 0) return 0;
        const int w = wr(user, (const uint8_t *)p, n);
        if (w == 0) return 0;
        err = "write callback failed";
        return w < 0 ? w : FCX_ERR_ARG;
    }
};

// prefix: what every format message of the file starts with ("repair file: ", "digest file: ")
struct ReadBase {
    const char *prefix;
    fcx_read_fn rd;
    void *user;
    std::string err;

    ReadBase(const char *p, fcx_read_fn r, void *u) : prefix(p), rd(r), user(u) {}
    int bad(const char *why) {
        err = std::string(prefix) + why;
        return FCX_ERR_FORMAT;
    }
    // exactly n bytes, or an error; *eof (when given) is set instead when not one byte is left
    int get(uint8_t *p, uint64_t n, bool *eof = nullptr) {
        uint64_t got = 0;
        while (got < n) {
            const int64_t r = rd(user, p + got, n - got);
            if (r < 0) {
                err = "read callback failed";
                return FCX_ERR_ARG;
            }
            if (r == 0) break;
            got += (uint64_t)r;
        }
        if (got == 0 && eof) {
            *eof = true;
            return 0;
        }
        return got == n ? 0 : bad("truncated");
    }
    // behind the trailer the file ends
    int expect_end() {
        uint8_t one;
        bool eof = false;
        const int g = get(&one, 1, &eof);
        if (g && g != FCX_ERR_FORMAT) return g;
        if (!eof) return bad("bytes behind the trailer");
        return 0;
    }
};

}  // namespace fcx_sidecar

#endif  // FCX_SIDECAR_IO_H
