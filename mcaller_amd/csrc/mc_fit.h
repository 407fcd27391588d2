// What the `--train` fit units (mc_train.hip, mc_forest_fit.hip, mc_svm_fit.hip, mc_simple_fit.hip) share on the host side of an entry
// point, and two small device helpers.  Included by those four units only, hence the unnamed namespace: nothing here is linked
// across units.  An entry point refuses its arguments (-12) before it touches the device, then
//
//     Pool pool("mc_x_fit");                      // device allocations (mc_own.h), freed when the entry point returns by any path
//     T *d = pool.get<T>(n); ...
//     if (!pool.ok) return -10;                   // (the message is set)
//     Xfer x("mc_x_fit", stream);                 // the first HIP error on this stream; every member is a no-op after one
//     x.up(d, h, n); x.zero(d2, m); x.launch(kernel, grid, block, lds, args); x.down(h2, d2, m); x.sync();
//     if (!x.ok()) return x.fail();               // "mc_x_fit failed: <text>", -10
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mcaller_hip.h"
#include "mc_own.h"

int mc_internal_device(const mc_ctx *c);
hipStream_t mc_internal_stream(const mc_ctx *c);

namespace {

// a fit of one call: its training and held-out rows as ranges of the call's index arrays, and its seed
struct FitJob {
    int64_t tr_off, n_tr, va_off, n_va;
    uint64_t seed;
};

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct Xfer {
    const char *who;
    hipStream_t st;
    hipError_t e = hipSuccess;
    Xfer(const char *w, hipStream_t s) : who(w), st(s) {}
    bool ok() const { return e == hipSuccess; }
    template <typename T>
    void up(T *dst, const T *src, size_t n) {
        if (ok() && n) e = hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st);
    }
    template <typename T>
    void zero(T *dst, size_t n) {
        if (ok() && n) e = hipMemsetAsync(dst, 0, n * sizeof(T), st);
    }
    template <typename H, typename T>
    void down(H *dst, const T *src, size_t n) {             // (H: int64_t for a device's long long, and the like)
        static_assert(sizeof(H) == sizeof(T), "host and device elements of one size");
        if (ok() && n) e = hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st);
    }
    template <typename K, typename... Args>
    void launch(K kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
        if (!ok()) return;
        hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
        e = hipGetLastError();
    }
    void sync() {
        if (ok()) e = hipStreamSynchronize(st);
    }
    int fail() const {
        mc_set_error("%s failed: %s", who, hipGetErrorString(e));
        return -10;
    }
};

// hipSetDevice for the context -> 0, or -10 with the error set
inline int select_device(const char *who, const mc_ctx *c) {
    if (hipSetDevice(mc_internal_device(c)) == hipSuccess) return 0;
    mc_set_error("%s: hipSetDevice failed", who);
    return -10;
}

// idx[lo, hi) are rows of the matrix -> 0, or -12 with the error set
inline int check_rows(const char *who, const int32_t *idx, int64_t lo, int64_t hi, int64_t n_samples) {
    for (int64_t i = lo; i < hi; ++i)
        if (idx[i] < 0 || idx[i] >= n_samples) { mc_set_error("%s: row index out of range", who); return -12; }
    return 0;
}

// A call's matrix and jobs: y in {0, 1} and X finite (as float64, or after the cast to float32); offsets that start at 0; per job
// min_tr .. max_rows training rows (min_tr 1 or 2) and 0 .. max_rows held-out rows, every index a row of the matrix, and, if
// both_classes, training rows of both classes.  n_neg[j], if given: job j's training rows of class 0.  -> 0, or -12 with the error
// set.  (mc_mlp_fit takes jobs without rows and does not look at X or y: it keeps a loop of its own over check_rows.)
inline int check_jobs(const char *who, const double *X, const uint8_t *y, int64_t n_samples, int d, int32_t n_jobs,
                      const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx,
                      int64_t max_rows, int min_tr, bool both_classes, bool x_as_float32, int64_t *n_neg) {
    for (int64_t i = 0; i < n_samples; ++i) {
        if (y[i] > 1) { mc_set_error("%s: labels must be 0 or 1", who); return -12; }
        for (int f = 0; f < d; ++f)
            if (!(x_as_float32 ? std::isfinite((float)X[i * d + f]) : std::isfinite(X[i * d + f]))) {
                mc_set_error("%s: X holds a value that is not finite%s", who, x_as_float32 ? " in float32" : "");
                return -12;
            }
    }
    if (train_off[0] != 0 || val_off[0] != 0) { mc_set_error("%s: offsets must start at 0", who); return -12; }
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t ntr = train_off[j + 1] - train_off[j], nva = val_off[j + 1] - val_off[j];
        if (ntr < min_tr || ntr > max_rows || nva < 0 || nva > max_rows || train_off[j + 1] > ((int64_t)1 << 31) ||
            val_off[j + 1] > ((int64_t)1 << 31)) {
            mc_set_error("%s: bad offsets for job %d (every job needs %straining rows)", who, j, min_tr > 1 ? "two " : "");
            return -12;
        }
        if (check_rows(who, train_idx, train_off[j], train_off[j + 1], n_samples)) return -12;
        int64_t cnt[2] = {0, 0};
        for (int64_t i = train_off[j]; i < train_off[j + 1]; ++i) ++cnt[y[train_idx[i]]];
        if (both_classes && (cnt[0] == 0 || cnt[1] == 0)) {
            mc_set_error("%s: job %d has training rows of one class only", who, j);
            return -12;
        }
        if (nva > 0 && !val_idx) { mc_set_error("%s: a required pointer is NULL", who); return -12; }
        if (check_rows(who, val_idx, val_off[j], val_off[j + 1], n_samples)) return -12;
        if (n_neg) n_neg[j] = cnt[0];
    }
    return 0;
}

}  // namespace
