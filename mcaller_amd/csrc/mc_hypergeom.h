// mc_hypergeom.h -- the upper tail of the hypergeometric distribution, for a host and a device compiler alike: what evaluate.py's
// "site d" tables need for the expectation of a site's call at a subsampled depth (mcaller_amd/evaluate.py: draw d of a site's N
// reads, K of them called methylated, without replacement; T = P(X >= k)).  C ABI: mc_hypergeom_tail / mc_hypergeom_tail_many (the
// host build, mc_format.cpp), mc_hypergeom_tail_device (a lane per case, bed/mc_bedsum.hip); tests/test_hypergeom.py and
// tests/test_gpu_evaluate.py hold both against exact rationals.  No kernel is defined here, and no lgamma: the weights come from the
// ratio recurrence, in integers and fp64 products.
//
//   p(x)     = C(K, x) C(N - K, d - x) / C(N, d)        lo = max(0, d - (N - K)) <= x <= hi = min(K, d)
//   w(x)     = p(x) / p(m), m the mode floor((d + 1)(K + 1) / (N + 2)) kept inside [lo, hi]; w(m) = 1 and
//              w(x + 1) = w(x) a / b,  a = (K - x)(d - x),             b = (x + 1)(N - K - d + x + 1)       (upwards from m)
//              w(x - 1) = w(x) a / b,  a = x (N - K - d + x),          b = (K - x + 1)(d - x + 1)           (downwards from m)
//              With N < 2^31 and d <= HG_MAX_D = 2^20 every a and b is an integer below 2^53, formed in 64-bit integers and
//              converted without rounding; 1 <= a and 1 <= b inside the range.
//   tail     = sum_{x >= k} w / sum_x w, both sums in the order of the walk (m, m + 1 .. hi, then m - 1 .. lo), every term positive
//   trivial  : 1 when k <= lo, 0 when k > hi, exactly (no arithmetic)
//   round4   = rint(v * 10000) / 10000: the fp64 operations of np.round(v, 4)
//   tie test = could rint(h * 10000) differ from rint(v * 10000) for some h with |h - v| <= err?  (monotone: the two ends decide)
//
// The bound `err` on |tail - exact|, DERIVED (u = 2^-53; gamma(n) = n u / (1 - n u)):
//
// (1) A weight.  One step is two roundings, fl(fl(w a) / b) with a and b exact, so s steps from the mode give
//         w'(x) = w(x) (1 + th),  |th| <= gamma(2 s),  s = |x - m| <= S, S the longer of the two walks.
//     Nothing overflows (w' stays near or below 1, a < 2^53) and nothing underflows: a walk STOPS at the first weight below
//     HG_TINY = 2^-900, so every step starts from a weight of at least 2^-900 and its product (>= 2^-900) and quotient
//     (>= 2^-953) are normal numbers; what the stop leaves out is (3).
// (2) A sum.  n positive terms added one after the other carry at most n - 1 roundings each: sum' = sum_i w'(x_i) (1 + e_i),
//     |e_i| <= gamma(n - 1).  With (1), each of the two sums is its exact value times (1 + r), |r| <= gamma(2 S + n - 1), n the
//     number of terms of the TOTAL (the tail has no more).  The quotient adds one rounding:
//         tail' = t (1 + q),  |q| <= gamma(M),  M = 2 (2 S + n - 1) + 1,  t the exact quotient of the kept terms
//     and from t <= tail' / (1 - gamma(M)):   |tail' - t| <= tail' g / (1 - g),  g = gamma(M).
// (3) The terms left out.  p is log-concave, so past the mode the weights only fall: the c terms a walk leaves out are each at
//     most the weight it stopped at, w_stop' / (1 - gamma(2 S)) <= 2 w_stop'.  With R <= 2 (c_up w_up' + c_dn w_dn') the sum of
//     what is left out and T >= 1 the exact total of the kept terms (w(m) = 1 is one of them):
//         |(A + R_t) / (T + R) - A / T| <= R / T <= R        (0 <= R_t <= R, A <= T).
// (4) The bound's own evaluation: a handful of fp64 operations, each within a factor (1 + u); M + 8 in place of M covers them
//     (the bound is a product of positive factors, so counting a rounding more per operation is enough).
//   =>  err = tail' g / (1 - g) + R,   g = gamma(M + 8).
// At d = 1024 that is at most 7e-13; profiles/hypergeom_error.json sets the largest derived err over a grid beside the largest
// MEASURED |tail - exact| of both builds (tools/hypergeom_error.py) -- the measurement lies under the bound, or (1)-(4) are wrong.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define HG_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define HG_HD inline
#endif

#define HG_MAX_N 2147483647LL            // N < 2^31
#define HG_MAX_D 1048576LL               // d <= 2^20: (N)(d) < 2^53
#define HG_TINY 1.1832913578315177e-271  // 2^-900: a walk stops below it, see (3)

// status of hg_tail
#define HG_OK 0
#define HG_BAD_ARGS 1                    // not 0 <= K <= N <= HG_MAX_N, 0 <= d <= min(N, HG_MAX_D): tail and err are NaN

// P(X >= k) for X ~ Hypergeometric(N, K, d) and the bound on its error; any k (k <= 0: 1, k > d: 0)
HG_HD int hg_tail(int64_t N, int64_t K, int64_t d, int64_t k, double *tail, double *err) {
    const double u = 1.1102230246251565e-16;
    if (!(N >= 0 && N <= HG_MAX_N && K >= 0 && K <= N && d >= 0 && d <= N && d <= HG_MAX_D)) {
        *tail = __builtin_nan(""); *err = __builtin_nan("");
        return HG_BAD_ARGS;
    }
    const int64_t lo = d - (N - K) > 0 ? d - (N - K) : 0, hi = K < d ? K : d;
    *err = 0.0;
    if (k <= lo) { *tail = 1.0; return HG_OK; }
    if (k > hi) { *tail = 0.0; return HG_OK; }
    int64_t m = ((d + 1) * (K + 1)) / (N + 2);
    m = m < lo ? lo : m > hi ? hi : m;
    const int64_t base = N - K - d;                                    // b's second factor is base + x + 1 >= 1 for x >= lo
    double total = 1.0, part = m >= k ? 1.0 : 0.0, rest = 0.0;
    int64_t s_up = 0, s_dn = 0;
    double w = 1.0;
    for (int64_t x = m; x < hi; ++x) {                                 // upwards: w(x + 1) from w(x)
        w = w * (double)((K - x) * (d - x)) / (double)((x + 1) * (base + x + 1));
        if (w < HG_TINY) { rest += (double)(hi - x) * w; break; }
        ++s_up;
        total += w;
        if (x + 1 >= k) part += w;
    }
    w = 1.0;
    for (int64_t x = m; x > lo; --x) {                                 // downwards: w(x - 1) from w(x)
        w = w * (double)(x * (base + x)) / (double)((K - x + 1) * (d - x + 1));
        if (w < HG_TINY) { rest += (double)(x - lo) * w; break; }
        ++s_dn;
        total += w;
        if (x - 1 >= k) part += w;
    }
    const double t = part / total;
    const double S = (double)(s_up > s_dn ? s_up : s_dn), n = (double)(s_up + s_dn + 1);
    const double Mu = (2.0 * (2.0 * S + n - 1.0) + 1.0 + 8.0) * u;     // (M + 8) u
    const double g = Mu / (1.0 - Mu);
    *tail = t;
    *err = t * g / (1.0 - g) + 2.0 * rest;
    return HG_OK;
}

HG_HD double hg_round4(double v) { return rint(v * 10000.0) / 10000.0; }

// could np.round(h, 4) differ from np.round(v, 4) for an h within err of v -- another ten-thousandth, or the other zero ("-0.0")?
// (err >= 0; a NaN anywhere: yes)
HG_HD bool hg_tie4_between(double lo_v, double hi_v) {
    const double lo = rint(lo_v * 10000.0), hi = rint(hi_v * 10000.0);
    return !(lo == hi) || __builtin_signbit(lo) != __builtin_signbit(hi);
}
HG_HD bool hg_tie4(double v, double err) { return hg_tie4_between(v - err, v + err); }
