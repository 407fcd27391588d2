// mc_fisher.h -- Fisher's exact test on the counts of two samples, for a host and a device compiler alike: what compare_genomes
// --fisher prints for a site whose lines say K1 methylated reads of n1 and K2 of n2 (mcaller_amd/compare_genomes.py: fisher_nlp is
// the definition, in exact rationals).  C ABI: mc_fisher_exact / mc_fisher_exact_many (the host build, mc_format.cpp),
// mc_fisher_exact_device (a lane per case, compare/mc_cmpfdr.inc), mc_fisher_select; tests/test_fisher_bh.py and
// tests/test_gpu_compare_fdr.py hold both against the rationals.  No kernel is defined here, and no lgamma: the weights are
// mc_hypergeom.h's, from its ratio recurrence in integers below 2^53 and fp64 products.
//
//   X ~ Hypergeometric(N = n1 + n2, K = K1 + K2, d = n1), observed K1;  p(x), lo, hi, the mode m, w(x) = p(x) / p(m) and the two
//   recurrences as mc_hypergeom.h states them.
//   p        = sum of p(x) over the SELECTED x: those with p(x) <= p(K1) c, c the fp64 number 1 + 10^-7 (R's factor)
//            = A / T,  A = sum of w(x) over the selected x,  T = sum of w(x) over all x
//   log10p   = min(0, log10(fl(A' / T')))
//   Two walks, no array per lane: the first (m, m + 1 .. hi, then m - 1 .. lo, hg_tail's order and HG_TINY stop) adds T' and
//   notes w'(K1); the second repeats the kept steps -- the same operations on the same numbers, so the same weights bit for
//   bit -- and adds the selected ones to A'.  When every x is selected A' and T' are one sum: the quotient is exactly 1 and
//   log10p exactly 0.
//   trivial  : K = 0, K = N or lo == hi (one value of X): log10p = 0.0, bound = 0, exactly (no arithmetic)
//
// The bound on |log10p - log10(exact p)|, DERIVED (u = 2^-53; gamma(n) = n u / (1 - n u)); (1)-(3) are mc_hypergeom.h's:
//
// (1) A weight: w'(x) = w(x) (1 + th), |th| <= gamma(2 s), s = |x - m| <= S, S the longer of the two walks; nothing overflows or
//     underflows because a walk stops at the first weight below HG_TINY = 2^-900.
// (2) The two sums: each is a sum of positive terms of the walk added one after the other, at most n of them (n the terms of
//     T'), so A' = A (1 + r_A), T' = T (1 + r_T), |r| <= gamma(2 S + n - 1).  Both errors are RELATIVE, however small A is: the
//     bound holds in the far tail as it does at p = 1/2.  The quotient adds one rounding:
//         fl(A' / T') = (A / T) (1 + q),  |q| <= gamma(M),  M = 2 (2 S + n - 1) + 1
//         |log10(1 + q)| <= g / ((1 - g) ln 10),  g = gamma(M).
// (3) The terms left out.  A walk stops only below HG_TINY, and K1's weight was kept (otherwise (5)), so every weight left out is
//     below w(K1): in exact arithmetic all of them are selected, and the exact p is (A + R) / (T + R), R <= 2 rest' the mass left
//     out (rest' = c_up w_up' + c_dn w_dn' as computed).  (A + R) / (T + R) >= A / T and
//         (A + R) / (T + R) / (A / T) <= 1 + R / A   =>   the logarithm moves by at most (R / A) / ln 10 <= 0.87 rest' / A'
//     with the roundings of A' and rest' taken into 0.9.  Above the far tail this is nothing: log10 p >= -250 and T <= 2^20 give
//     A >= 10^-250, while at most 2^20 terms of twice the stop weight are left out, R < 2.5e-265: 2.5e-15 of such a p.
// (4) log10 itself.  The host's libm and the device's log10 are within 2 ulp of the logarithm of their argument, and the
//     reference (the fp64 number nearest to log10 of the exact p) within half an ulp of its own: 8 u |log10p| covers them.
//     The bound's own evaluation is a handful of fp64 operations on positive factors: M + 8 in place of M covers them.
//   =>  bound = 0.4343 g / (1 - g) + 0.9 rest' / A' + 8 u |log10p|,   g = gamma(M + 8).
//     At 8192 pooled reads that is below 4e-12; profiles/fisher_error.json sets the largest derived bound over a grid beside the
//     largest MEASURED |log10p - exact| of both builds (tools/fisher_error.py) -- the measurement lies under the bound, or
//     (1)-(4) are wrong.
// (5) FE_FAR_TAIL: log10p < FE_LOG10P_MIN = -250 (the value and the bound still stand, by (2): the caller decides what to do with
//     a p that small), or K1's own weight fell below HG_TINY and was never reached: log10p = -inf, bound = +inf.
// (6) FE_SELECT: the selection compares w'(x) with thr' = fl(w'(K1) c).  By (1), w'(x) / thr' is the exact ratio w(x) / (w(K1) c)
//     within a relative gamma(2 s_x + 2 s_K1 + 1) <= gamma(4 S + 1); the predicate's own arithmetic takes it to
//         e = gamma(4 S + 8).
//     A weight with |w'(x) - thr'| <= e thr' could be selected in one arithmetic and not in the other: the status says so and the
//     caller declines.  Everywhere else the computed selection IS the exact one.  The exact ties of a symmetric table (n1 = n2:
//     w(x) = w(K - x)) have a computed ratio within 10^-13 of 1 -- 10^-7 away from c, six orders beyond e <= 5e-10 -- and are
//     selected by both.
#pragma once
#include "mc_hypergeom.h"

#define FE_OK 0
#define FE_BAD_ARGS 1                    // not 0 <= K1 <= n1 <= HG_MAX_D, 0 <= K2 <= n2, n1 + n2 <= HG_MAX_N: NaN twice
#define FE_FAR_TAIL 2                    // see (5)
#define FE_SELECT 4                      // see (6)

#define FE_LOG10P_MIN (-250.0)
#define FE_FACTOR 1.0000001              // c: the fp64 number nearest to 1 + 10^-7

// K of a line of n reads whose frac field reads f: make_bed wrote str(np.mean(labels)) = K / n in fp64, so K = rint(f n) and the line
// is sound iff 0 <= K <= n and K / n == f (compare_genomes.site_counts, the same operations)
HG_HD bool fe_count(double f, int64_t n, int64_t *K) {
    if (n < 1 || !(fabs(f) < INFINITY)) return false;
    const double k = rint(f * (double)n);
    if (!(k >= 0.0 && k <= (double)n) || k / (double)n != f) return false;
    *K = (int64_t)k;
    return true;
}

// e of (6) for walks of at most S steps
HG_HD double fe_select_err(double S) {
    const double u = 1.1102230246251565e-16, k = (4.0 * S + 8.0) * u;
    return k / (1.0 - k);
}

// is the weight w selected beside the observed weight w_obs (1: yes, 0: no), and in bit 1 (+2): could the exact comparison say
// otherwise?  S: the longer walk
HG_HD int fe_select(double w, double w_obs, double S) {
    const double thr = w_obs * FE_FACTOR;
    return (w <= thr ? 1 : 0) | (fabs(w - thr) <= fe_select_err(S) * thr ? 2 : 0);
}

// log10 of the two-sided p of Fisher's exact test on the table (K1, n1 - K1; K2, n2 - K2), the bound on its error and the status bits
HG_HD void fe_log10p(int64_t K1, int64_t n1, int64_t K2, int64_t n2, double *log10p, double *bound, int *status) {
    const double u = 1.1102230246251565e-16;
    if (!(n1 >= 0 && n2 >= 0 && K1 >= 0 && K1 <= n1 && K2 >= 0 && K2 <= n2 && n1 <= HG_MAX_D && n2 <= HG_MAX_N && n1 + n2 <= HG_MAX_N)) {
        *log10p = __builtin_nan(""); *bound = __builtin_nan(""); *status = FE_BAD_ARGS;
        return;
    }
    const int64_t N = n1 + n2, K = K1 + K2, d = n1;
    const int64_t lo = d - (N - K) > 0 ? d - (N - K) : 0, hi = K < d ? K : d;
    *log10p = 0.0; *bound = 0.0; *status = FE_OK;
    if (K == 0 || K == N || lo == hi) return;
    int64_t m = ((d + 1) * (K + 1)) / (N + 2);
    m = m < lo ? lo : m > hi ? hi : m;
    const int64_t base = N - K - d;
    double total = 1.0, rest = 0.0, w_obs = K1 == m ? 1.0 : 0.0;
    int64_t s_up = 0, s_dn = 0;
    double w = 1.0;
    for (int64_t x = m; x < hi; ++x) {                                 // hg_tail's walk: the total, and K1's weight on the way
        w = w * (double)((K - x) * (d - x)) / (double)((x + 1) * (base + x + 1));
        if (w < HG_TINY) { rest += (double)(hi - x) * w; break; }
        ++s_up;
        total += w;
        if (x + 1 == K1) w_obs = w;
    }
    w = 1.0;
    for (int64_t x = m; x > lo; --x) {
        w = w * (double)(x * (base + x)) / (double)((K - x + 1) * (d - x + 1));
        if (w < HG_TINY) { rest += (double)(x - lo) * w; break; }
        ++s_dn;
        total += w;
        if (x - 1 == K1) w_obs = w;
    }
    if (!(w_obs > 0.0)) {                                              // (5): K1 lies beyond the stop
        *log10p = -INFINITY; *bound = INFINITY; *status = FE_FAR_TAIL;
        return;
    }
    const double S = (double)(s_up > s_dn ? s_up : s_dn), n = (double)(s_up + s_dn + 1);
    int near = 0;
    int sel = fe_select(1.0, w_obs, S);                                // the kept steps again: the selected weights
    near |= sel;
    double part = (sel & 1) ? 1.0 : 0.0;
    w = 1.0;
    for (int64_t x = m; x < m + s_up; ++x) {
        w = w * (double)((K - x) * (d - x)) / (double)((x + 1) * (base + x + 1));
        sel = fe_select(w, w_obs, S);
        near |= sel;
        if (sel & 1) part += w;
    }
    w = 1.0;
    for (int64_t x = m; x > m - s_dn; --x) {
        w = w * (double)(x * (base + x)) / (double)((K - x + 1) * (d - x + 1));
        sel = fe_select(w, w_obs, S);
        near |= sel;
        if (sel & 1) part += w;
    }
    const double l = log10(part / total), L = l < 0.0 ? l : 0.0;
    const double Mu = (2.0 * (2.0 * S + n - 1.0) + 1.0 + 8.0) * u;     // (M + 8) u
    const double g = Mu / (1.0 - Mu);
    *log10p = L;
    *bound = 0.4343 * g / (1.0 - g) + 0.9 * rest / part + 8.0 * u * -L;
    *status = ((near & 2) ? FE_SELECT : 0) | (L < FE_LOG10P_MIN ? FE_FAR_TAIL : 0);
}
