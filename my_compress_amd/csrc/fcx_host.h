// fcx_host.h — the host layer the C ABI files share (no device code): the last-error helpers,
// owned device / pinned memory, streams and events, the stage-time recorder of the profiled paths and the deleter of
// per-thread and lazily made objects.  DESIGN.md, "host layer".
#ifndef FCX_HOST_H
#define FCX_HOST_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <utility>

#include "fcx.h"

namespace fcx {

// ---- errors: the text goes to fcx_last_error() (fcx_capi.hip), the code to the caller ----------
void set_last_error(const std::string &m);
inline int fail(int code, const std::string &msg) {
    set_last_error(msg);
    return code;
}
#define FCX_HIP(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fcx::fail(FCX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define FCX_TRY(expr)          \
    do {                       \
        int rc_ = (expr);      \
        if (rc_) return rc_;   \
    } while (0)

// ---- owned memory: device (hipMalloc) or pinned host (hipHostMalloc) ---------------------------
// Frees what it holds when it goes; movable, so a struct of them is dropped as a whole by assigning
// a fresh one.  Sizes are bytes; a request of 0 allocates 16.
template <typename T, bool kPinned>
struct Buf {
    T *p = nullptr;
    uint64_t bytes = 0;   // as requested
    Buf() = default;
    Buf(Buf &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~Buf() { release(); }
    void release() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }
    // drops what it holds, then allocates: for the callers that report a failure as FCX_ERR_HIP
    hipError_t alloc(uint64_t n) {
        release();
        const uint64_t req = n ? n : 16;
        const hipError_t e = kPinned ? hipHostMalloc((void **)&p, req, hipHostMallocDefault) : hipMalloc((void **)&p, req);
        if (e != hipSuccess) p = nullptr;
        else bytes = n;
        return e;
    }
    // holds >= n bytes afterwards; allocates anew (contents lost) only when it holds fewer
    int reserve(uint64_t n, const char *what) {
        if (p && n <= bytes) return FCX_OK;
        const hipError_t e = alloc(n);
        if (e == hipSuccess) return FCX_OK;
        return fail(FCX_ERR_NOMEM, std::string(kPinned ? "hipHostMalloc " : "hipMalloc ") + what + ": " + hipGetErrorString(e));
    }
    operator T *() const { return p; }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

// ---- owned stream / event ----------------------------------------------------------------------
// One handle each: move-only, converts to it, destroys it when it goes.  create(flags) drops what
// it holds and returns the hipError_t, so a caller keeps its own error code and text.
template <typename H, hipError_t (*Make)(H *, unsigned), hipError_t (*Drop)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) {
            release();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Handle() { release(); }
    void release() {
        if (h) (void)Drop(h);
        h = nullptr;
    }
    hipError_t create(unsigned flags = 0) {
        release();
        const hipError_t e = Make(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

// unique_ptr deleter that calls Fn: contexts a host thread keeps for itself
// (thread_local std::unique_ptr<fcx_dctx, Calls<fcx_dctx_destroy>>, gone at thread exit) and parts
// whose type is complete in one file only
template <auto Fn>
struct Calls {
    template <typename T> void operator()(T *p) const { Fn(p); }
};

// ---- stage times of a profiled call ------------------------------------------------------------
// Stage k runs between events k and k + 1 (the launchers record into events() themselves).  A
// call starts with reset() and makes its table visible to the *_stage queries with publish(): at
// once with the events still to read (lazy: the first query waits for them), or at its end after
// add() has summed the spans itself (eager: FCX8 reuses the events per batch).
struct StageTimes {
    static constexpr int kStages = 11;
    hipEvent_t ev[kStages + 1] = {};
    const char *const *names = nullptr;
    int n = 0;           // stages of the published table; 0: the last call was not profiled
    bool lazy = false;   // the events are not read yet
    float ms[kStages] = {};

    explicit StageTimes(int stages) {
        for (int i = 0; i <= stages; i++) (void)hipEventCreate(&ev[i]);
    }
    StageTimes(const StageTimes &) = delete;
    StageTimes &operator=(const StageTimes &) = delete;
    ~StageTimes() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void reset() {
        n = 0;
        lazy = false;
        for (float &v : ms) v = 0;
    }
    void publish(const char *const *table, int stages, bool lazy_read = false) {
        names = table;
        n = stages;
        lazy = lazy_read;
    }
    hipEvent_t *events() { return ev; }
    void mark(int i, hipStream_t st) { (void)hipEventRecord(ev[i], st); }
    // ms[k] += the span of stage k, first <= k < last, once event `last` has passed
    int add(int first, int last) {
        FCX_HIP(hipEventSynchronize(ev[last]));
        for (int k = first; k < last; k++) {
            float v = 0;
            FCX_HIP(hipEventElapsedTime(&v, ev[k], ev[k + 1]));
            ms[k] += v;
        }
        return FCX_OK;
    }
    // stage i of the published table (0 <= i < n)
    int stage(int i, const char **name, float *out) {
        if (lazy) {
            for (float &v : ms) v = 0;
            FCX_TRY(add(0, n));
            lazy = false;
        }
        if (name) *name = names[i];
        if (out) *out = ms[i];
        return FCX_OK;
    }
};

}  // namespace fcx

#endif  // FCX_HOST_H
