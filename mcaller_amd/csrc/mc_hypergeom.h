// mc_hypergeom.h -- the upper tail of the hypergeometric distribution, for a host and a device compiler alike: what evaluate.py's
// "site d" tables need for the expectation of a site's call at a subsampled depth (mcaller_amd/evaluate.py: draw d of a site's N
// reads, K of them called methylated, without replacement; T = P(X >= k)).  C ABI: mc_hypergeom_tail / mc_hypergeom_tail_many (the
// host build, mc_format.cpp), mc_hypergeom_tail_device (a lane per case, bed/mc_bedsum.hip); tests/test_hypergeom.py and
// tests/test_gpu_evaluate.py hold both against exact rationals.  No kernel is defined here, and no lgamma: the weights come from the
// ratio recurrence, in integers and fp64 products.  All 101 tails of a (N, K, d) at once: hg_masses, below (C ABI:
// mc_hypergeom_masses / _many, mc_hypergeom_masses_device; eval/mc_evalcalls.hip's ke_expect runs it per (site, depth)).
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
//
// hg_masses: all 101 tails of one (N, K, d).  A "site d" table asks for P(X >= k_min(d, j)), j = 0 .. 100, k_min(d, j) the smallest
// x with x / d >= j / 100 in fp64.  tests/test_evaluate.py::test_k_min_at_100_7_and_on_every_depth holds that fp64 rule equal to
// the rule of the rationals for every d <= 1024: x passes threshold j iff 100 x >= j d, so the number of thresholds x passes is
//     c(x) = #{j in 0 .. 100 : 100 x >= j d} = (100 x) / d + 1   in integers (0 <= x <= d: 1 <= c <= 101),
// x >= k_min(d, j) iff c(x) > j, and with mass[c] the probability of the bucket {x : c(x) = c}
//     P(X >= k_min(d, j)) = tail_j = sum_{c > j} mass[c].
// The weights are those of hg_tail, walked in its order (mode, up, down, the same HG_TINY stop) -- once for the total and once more
// to hand each bucket out as it closes (c rises with x, so a bucket is a run of the walk; the mode's bucket is closed by the
// downward walk, which starts from what the upward walk left in it): no array of 102 sums per lane on the device, and two walks
// in place of 101.  mass'[c] = fl(B'(c) / T'), B' the bucket's sum in the order of the walk, T' hg_tail's total.
// The bound `err` on sum_c |mass'[c] - mass[c]|, which bounds the error of every tail_j formed from the masses exactly, DERIVED:
// (1) holds for every weight as it stands.  (2): a bucket's terms are positive terms of the walk added one after the other, at most
//     n of them, so B'(c) = B(c) (1 + r_c), |r_c| <= gamma(2 S + n - 1), and T' = T (1 + r) as before; the division adds one rounding
//     a bucket:  mass'[c] = (B(c) / T) (1 + q_c),  |q_c| <= gamma(M),  M = 2 (2 S + n - 1) + 1.  The kept terms' buckets sum to T:
//         sum_c |mass'[c] - B(c) / T| <= gamma(M) sum_c B(c) / T = gamma(M).
// (3): with R_c the left-out weight of bucket c, sum_c R_c = R <= 2 (c_up w_up' + c_dn w_dn') and T >= 1:
//         sum_c |(B(c) + R_c) / (T + R) - B(c) / T| <= sum_c (R_c T + B(c) R) / (T (T + R)) = 2 R / (T + R) <= 2 R.
// (4) as above.   =>  err = g + 2 R = g + 4 rest',  g = gamma(M + 8),  rest' = c_up w_up' + c_dn w_dn' as computed.
// lo == hi (d = N, K = 0, K = N, ...): one bucket of mass exactly 1, err = 0, no arithmetic.  (d = 0: the one mass goes to bucket 1.)
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

#define HG_BUCKETS 102                   // mass[0 .. 101]; mass[0] is always 0

HG_HD int hg_bucket(int64_t x, int64_t d) { return d > 0 ? (int)((100 * x) / d) + 1 : 1; }

// The bucket masses of X ~ Hypergeometric(N, K, d): sink.put(c, mass) once for every bucket c in 1 .. 101 that holds an x of
// [lo, hi] whose weight the walk kept (every other bucket's mass is 0), *err the bound on sum_c |mass'[c] - mass[c]|.
// Bad arguments: nothing is put, *err is NaN.
template <class Sink>
HG_HD int hg_masses_to(int64_t N, int64_t K, int64_t d, Sink &sink, double *err) {
    const double u = 1.1102230246251565e-16;
    if (!(N >= 0 && N <= HG_MAX_N && K >= 0 && K <= N && d >= 0 && d <= N && d <= HG_MAX_D)) {
        *err = __builtin_nan("");
        return HG_BAD_ARGS;
    }
    const int64_t lo = d - (N - K) > 0 ? d - (N - K) : 0, hi = K < d ? K : d;
    *err = 0.0;
    if (lo == hi) { sink.put(hg_bucket(lo, d), 1.0); return HG_OK; }
    int64_t m = ((d + 1) * (K + 1)) / (N + 2);
    m = m < lo ? lo : m > hi ? hi : m;
    const int64_t base = N - K - d;
    double total = 1.0, rest = 0.0;
    int64_t s_up = 0, s_dn = 0;
    double w = 1.0;
    for (int64_t x = m; x < hi; ++x) {                                 // hg_tail's walk: the total
        w = w * (double)((K - x) * (d - x)) / (double)((x + 1) * (base + x + 1));
        if (w < HG_TINY) { rest += (double)(hi - x) * w; break; }
        ++s_up;
        total += w;
    }
    w = 1.0;
    for (int64_t x = m; x > lo; --x) {
        w = w * (double)(x * (base + x)) / (double)((K - x + 1) * (d - x + 1));
        if (w < HG_TINY) { rest += (double)(x - lo) * w; break; }
        ++s_dn;
        total += w;
    }
    const int cm = hg_bucket(m, d);                                    // the kept steps again: the buckets as they close
    int c = cm;
    double acc = 1.0, first = 1.0;
    w = 1.0;
    for (int64_t x = m; x < m + s_up; ++x) {
        w = w * (double)((K - x) * (d - x)) / (double)((x + 1) * (base + x + 1));
        const int cx = hg_bucket(x + 1, d);
        if (cx != c) {
            if (c == cm) first = acc; else sink.put(c, acc / total);
            c = cx; acc = 0.0;
        }
        acc += w;
    }
    if (c == cm) first = acc; else sink.put(c, acc / total);
    c = cm; acc = first;
    w = 1.0;
    for (int64_t x = m; x > m - s_dn; --x) {
        w = w * (double)(x * (base + x)) / (double)((K - x + 1) * (d - x + 1));
        const int cx = hg_bucket(x - 1, d);
        if (cx != c) { sink.put(c, acc / total); c = cx; acc = 0.0; }
        acc += w;
    }
    sink.put(c, acc / total);
    const double S = (double)(s_up > s_dn ? s_up : s_dn), n = (double)(s_up + s_dn + 1);
    const double Mu = (2.0 * (2.0 * S + n - 1.0) + 1.0 + 8.0) * u;     // (M + 8) u
    *err = Mu / (1.0 - Mu) + 4.0 * rest;
    return HG_OK;
}

struct HgMassArray {
    double *mass;
    HG_HD void put(int c, double v) { mass[c] = v; }
};

// mass[0 .. 101] (HG_BUCKETS doubles) and the bound; bad arguments: NaN everywhere
HG_HD int hg_masses(int64_t N, int64_t K, int64_t d, double *mass, double *err) {
    for (int c = 0; c < HG_BUCKETS; ++c) mass[c] = 0.0;
    HgMassArray sink = {mass};
    const int st = hg_masses_to(N, K, d, sink, err);
    if (st != HG_OK)
        for (int c = 0; c < HG_BUCKETS; ++c) mass[c] = __builtin_nan("");
    return st;
}

HG_HD double hg_round4(double v) { return rint(v * 10000.0) / 10000.0; }

// could np.round(h, 4) differ from np.round(v, 4) for an h within err of v -- another ten-thousandth, or the other zero ("-0.0")?
// (err >= 0; a NaN anywhere: yes)
HG_HD bool hg_tie4_between(double lo_v, double hi_v) {
    const double lo = rint(lo_v * 10000.0), hi = rint(hi_v * 10000.0);
    return !(lo == hi) || __builtin_signbit(lo) != __builtin_signbit(hi);
}
HG_HD bool hg_tie4(double v, double err) { return hg_tie4_between(v - err, v + err); }
