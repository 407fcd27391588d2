// mc_own.h -- the owners of what the host side takes from the HIP runtime: device allocations (Pool), a pinned block (Pinned), one
// that grows with the results handed out in it (Grown), an event (Event), a stream (Stream).  Each releases what it holds in its
// destructor, so a function that returns early (HIP_TRY) and a context that is deleted free everything on every path.  hipFree, hipHostFree, hipEventDestroy and hipStreamDestroy are called
// here and in two other places under csrc/: mc_host_alloc's block cache (mc_common.cpp: process-wide host buffers that fall back
// to malloc, no context owns them) and mc_debug_tanh32_max_err (mc_classify.hip, a kernel unit: eight bytes around one launch).
// Included by mc_ctx.h (the context's units; through it by mc_lines.h and mc_textfeed.h, the seven file pipelines' units) and by
// mc_fit.h (the --train fits).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

void mc_set_error(const char *fmt, ...);

// -> 0, or -10 with the error set
inline int mc_hip_rc(hipError_t e, const char *what) {
    if (e != hipSuccess) mc_set_error("%s failed: %s", what, hipGetErrorString(e));
    return e == hipSuccess ? 0 : -10;
}

// device allocations that live and die together; a re-size is clear() followed by the allocations
struct Pool {
    const char *who;
    bool ok = true;                             // false once an allocation has failed (until clear())
    std::vector<void *> p;
    explicit Pool(const char *w) : who(w) {}
    Pool(const Pool &) = delete;
    ~Pool() { clear(); }
    void clear() {
        for (void *q : p) (void)hipFree(q);
        p.clear();
        ok = true;
    }
    template <typename T>
    T *get(size_t n) {                          // n elements (at least 256 bytes), or nullptr with the error set
        void *q = nullptr;
        const size_t bytes = std::max<size_t>(n * sizeof(T), 256);
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) {
            mc_set_error("%s: hipMalloc of %zu bytes failed: %s", who, n * sizeof(T), hipGetErrorString(e));
            ok = false;
            return nullptr;
        }
        p.push_back(q);
        // MCALLER_POISON: fill every fresh device allocation with 0xAB (tests: a kernel that reads memory nobody wrote shows up
        // as a mismatch or a fault instead of silently reading zero pages)
        static const bool poison = getenv("MCALLER_POISON") != nullptr;
        if (poison) { (void)hipMemset(q, 0xAB, bytes); (void)hipDeviceSynchronize(); }
        return (T *)q;
    }
    template <typename T>
    int get(T **dst, size_t n) {                // -> 0, or -10 with the error set
        *dst = get<T>(n);
        return *dst ? 0 : -10;
    }
};

// a block of pinned host memory (hipHostMalloc) and the address the GPU sees it at
struct Pinned {
    void *p = nullptr, *dev = nullptr;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    ~Pinned() { reset(); }
    void reset() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
    }
    int alloc(size_t bytes) {                   // (whatever it held is freed first) -> 0, or -10 with the error set
        reset();
        hipError_t e = hipHostMalloc(&p, std::max<size_t>(bytes, 256), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, p, 0);
        if (e == hipSuccess) return 0;
        mc_set_error("hipHostMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        reset();
        return -10;
    }
    template <typename T>
    T *get() const { return (T *)p; }
};

// a pinned block a result is handed out in, grown on demand.  It owns its capacity: the block and the figure cannot drift apart
struct Grown {
    Pinned block;
    size_t cap = 0;
    int need(size_t bytes) {                    // at least `bytes`, a quarter more when it has to grow (a failed allocation: nothing, cap 0)
        if (cap >= bytes) return 0;
        cap = 0;
        if (int rc = block.alloc(bytes + bytes / 4)) return rc;
        cap = bytes + bytes / 4;
        return 0;
    }
    void reset() {
        block.reset();
        cap = 0;
    }
    template <typename T>
    T *get() const { return block.get<T>(); }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int create(unsigned flags = hipEventDefault) { return mc_hip_rc(hipEventCreateWithFlags(&e, flags), "hipEventCreateWithFlags"); }
    operator hipEvent_t() const { return e; }
};

struct Stream {                                 // (non-blocking: none of the library's streams waits for the null stream)
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    int create() { return mc_hip_rc(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags"); }
    operator hipStream_t() const { return s; }
};
