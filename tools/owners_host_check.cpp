// owners_host_check.cpp — the owners of the host layer (fcx_host.h: Buf, Stream, Event) as a
// stand-alone host program, for a sanitizer build on a box with or without a device:
//
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//         -Imy_compress_amd/csrc tools/owners_host_check.cpp -o owners_host_check
//   ./owners_host_check
//
// Every create / alloc / reserve may fail (no device): an owner that failed holds nothing, and move,
// move-assign, release and a second release leave every owner consistent either way.  A marker
// value stands in for a handle where the moves themselves are followed; it never reaches the
// runtime.  Exit status 0 when every check holds; a sanitizer report is a failure.
#include <cstdio>
#include <utility>

#include "fcx_host.h"

namespace fcx {
static std::string g_last;
void set_last_error(const std::string &m) { g_last = m; }
}  // namespace fcx

using namespace fcx;

static int g_bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
            g_bad++;                                                 \
        }                                                            \
    } while (0)

// a Stream or an Event: create, move, move-assign over a live one, release twice
template <typename Owner, typename Raw>
static void check_handle(unsigned flags, const char *name) {
    Owner a;
    CHECK(!a);
    const hipError_t e = a.create(flags);
    CHECK((e == hipSuccess) == (a.h != nullptr));
    printf("%s: create %s\n", name, e == hipSuccess ? "made one" : hipGetErrorString(e));
    const Raw was = a;
    Owner b(std::move(a));
    CHECK(!a && (Raw)b == was);
    Owner c;
    (void)c.create(flags);   // (a live one, where there is a device: move-assign destroys it)
    c = std::move(b);
    CHECK(!b && (Raw)c == was);
    c = std::move(c);        // self-assign keeps it
    CHECK((Raw)c == was);
    (void)c.create(flags);   // create over a live one drops it first
    c.release();
    CHECK(!c);
    c.release();
    CHECK(!c);
    // the moves alone, with a marker no runtime call sees
    int marker = 0;
    Owner m;
    m.h = (Raw)(void *)&marker;
    Owner n(std::move(m));
    CHECK(!m && n.h == (Raw)(void *)&marker);
    Owner o;
    o = std::move(n);
    CHECK(!n && o.h == (Raw)(void *)&marker);
    o.h = nullptr;
}

template <typename B>
static void check_buf(const char *name) {
    B a;
    CHECK(!a.p && a.bytes == 0);
    const hipError_t e = a.alloc(4096);
    CHECK(e == hipSuccess ? (a.p && a.bytes == 4096) : (!a.p && a.bytes == 0));
    printf("%s: alloc %s\n", name, e == hipSuccess ? "made one" : hipGetErrorString(e));
    const int r = a.reserve(1 << 16, "owners_host_check");
    CHECK(r == FCX_OK ? (a.p && a.bytes == 1 << 16) : (r == FCX_ERR_NOMEM && !a.p && a.bytes == 0 && !g_last.empty()));
    auto *was = a.p;
    const uint64_t had = a.bytes;
    CHECK(a.reserve(16, "owners_host_check") == FCX_OK ? a.p != nullptr && (!was || (a.p == was && a.bytes == had)) : !a.p);
    was = a.p;
    B b(std::move(a));
    CHECK(!a.p && a.bytes == 0 && b.p == was);
    B c;
    (void)c.alloc(64);
    c = std::move(b);
    CHECK(!b.p && b.bytes == 0 && c.p == was);
    c = std::move(c);
    CHECK(c.p == was);
    c.release();
    CHECK(!c.p && c.bytes == 0);
    c.release();
    CHECK(!c.p && c.bytes == 0);
    unsigned char marker[16];
    B m;
    m.p = (decltype(m.p))marker;
    m.bytes = sizeof(marker);
    B n(std::move(m));
    CHECK(!m.p && m.bytes == 0 && n.p == (decltype(n.p))marker && n.bytes == sizeof(marker));
    B o;
    o = std::move(n);
    CHECK(!n.p && n.bytes == 0 && o.p == (decltype(o.p))marker && o.bytes == sizeof(marker));
    o.p = nullptr;
    o.bytes = 0;
}

// a struct of owners is dropped as a whole by assigning a fresh one (how fcx_dist drops its parts)
struct Part {
    Stream st;
    Event ev[3];
    DevBuf<uint8_t> d;
    PinnedBuf<uint64_t> h;
};

int main() {
    check_handle<Stream, hipStream_t>(hipStreamNonBlocking, "Stream");
    check_handle<Event, hipEvent_t>(hipEventDisableTiming, "Event");
    check_buf<DevBuf<uint8_t>>("DevBuf");
    check_buf<PinnedBuf<uint64_t>>("PinnedBuf");
    Part p;
    (void)p.st.create(hipStreamNonBlocking);
    for (auto &e : p.ev) (void)e.create();
    (void)p.d.alloc(1024);
    (void)p.h.alloc(1024);
    Part q;
    q = std::move(p);
    CHECK(!p.st && !p.ev[0] && !p.ev[2] && !p.d.p && !p.h.p);
    q = Part();
    CHECK(!q.st && !q.ev[1] && !q.d.p && !q.h.p);
    printf("owners_host_check: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
