// mc_tstat.h -- the one-sample Student t arithmetic of make_bed -p (make_bed.py:115-127: scipy.stats.ttest_1samp of a feature column
// against 0, then np.round(., 3)), for a host and a device compiler alike.  C ABI: mc_tstat (the host build, mc_format.cpp),
// mc_tstat_device (a lane per triple, bed/mc_bedsum.hip); tests/test_tstat.py and tests/test_gpu_bed_positions.py hold both against
// SciPy.  No kernel is defined here.
//
//   t        = mean / sqrt(var / n)                    var the sample variance (ddof = 1), n >= 2, var > 0
//   log10 p  = log10 of the two-sided tail 2 sf(|t|) with df = n - 1 degrees of freedom
//            = log10 I_x(df/2, 1/2) at x = df / (df + t^2), the regularised incomplete beta function, computed in the LOG domain:
//              ln I_x(a, b) = a ln x + b ln(1 - x) - ln B(a, b) - ln F(a, b, x, 1 - x)      (F: a continued fraction, ts_betacf)
//              with ln x = -log1p(t^2 / df) and 1 - x = t^2 / (df + t^2) formed without cancellation, so a p of 1e-290 keeps the
//              relative accuracy of its logarithm.  Near the centre (x > (a + 1) / (a + b + 2)) the fraction is that of the
//              complement, q = I_{1-x}(1/2, a), and ln p = log1p(-q).
//              ln B(a, 1/2) = ln sqrt(pi) - D(a), D(a) = lgamma(a + 1/2) - lgamma(a) from the DIFFERENCE of two Stirling series
//              (a shifted up to 16 or more first): no library lgamma takes part, and nothing cancels for df = 10^5.
//   round3   = rint(v * 1000) / 1000: the fp64 operations of np.round(v, 3)
//   tie test = could rint(h * 1000) differ from rint(v * 1000) for some h with |h - v| <= err?  (rint(. * 1000) is monotone, so the
//              two ends decide)
//
// The two error terms (what a caller adds up before it asks the tie test; every printed value is exact or the file is declined):
//
// (1) The function term, MEASURED.  |ts_log10_p(df, t) - log10(2 * scipy.special.stdtr(df, -|t|))| over the grid of
//     tests/tstat_grid.py (df 1 .. 10^5, |t| 10^-6 up to where log10 p reaches -290; profiles/tstat_error.json):
//         largest error / max(1, |log10 p|), host build against SciPy 1.15.3:   4.7e-15   (6478 points; at df 10^4, t 1.63)
//         TS_FN_BOUND (the bound used, x 64 and rounded up):                    4.0e-13   relative to max(1, |log10 p|)
//     The margin covers SciPy's own (unknown) error and the device's log / log1p / sqrt, which are not the host's bit for bit.
//
// (2) The moment term, DERIVED.  u = 2^-53; x_1 .. x_n the column, A = sum |x_i| / n, m the exact mean, SS the exact centred sum
//     of squares.  Any summation of n terms in any order (NumPy's pairwise one, a naive one) has an error of at most
//     (n - 1) u sum|terms| to first order; a compensated (two-sum) one of at most 2 u |sum| + n^2 u^2 sum|terms|: the device's own part
//     does not grow with the depth, the bound below covers BOTH sides with the order-free figure.
//         |mean' - m|   <= em = (n + 1) u A                                  (the sum, the division)
//         SS' = (SS + n d^2)(1 + th), d = mean' - m, |th| <= (n + 3) u       (x_i - mean' rounded, squared, summed; the shift
//                                                                             identity sum (x - m - d)^2 = SS + n d^2 is exact)
//      => rel. error of SS'  <= e_ss = (n + 3) u + n em^2 / SS
//         t = mean / sqrt(SS / (n - 1) / n): five more roundings (SciPy: mean of squares, * n / (n - 1), / n, sqrt, /), the square
//         root halves e_ss
//      => |t' - t| <= em / denom + |t| (e_ss / 2 + 8 u),   denom = sqrt(var / n)
//     ts_t_bound returns TWICE that: the host's t and the device's t each lie within one such distance of the exact t.
//     The bound on log10 p follows by evaluating ts_log10_p at |t| - bound and |t| + bound (it is monotone in |t|).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define TS_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define TS_HD inline
#endif

#define TS_FN_BOUND 4.0e-13              // see (1)
#define TS_LOG10P_MIN (-290.0)           // below: declined (the host's p underflows to 0 and prints inf somewhere beyond)
#define TS_CF_MAXIT 20000

// status bits of ts_stat
#define TS_OK 0
#define TS_BAD_N 1                       // n < 2: the host prints nan
#define TS_ZERO_VAR 2                    // var <= 0 or not finite, or mean not finite
#define TS_FAR_TAIL 4                    // log10 p < TS_LOG10P_MIN
#define TS_NO_CONVERGENCE 8              // the continued fraction did not settle (not seen on the grid)

// D(a) = lgamma(a + 1/2) - lgamma(a), a > 0
TS_HD double ts_lgamma_half_step(double a) {
    double shift = 0.0;                                               // Gamma(a + 1/2) / Gamma(a) = Gamma(a + 3/2) / Gamma(a + 1) * a / (a + 1/2)
    while (a < 16.0) { shift += log(a / (a + 0.5)); a += 1.0; }
    // lgamma(z) = (z - 1/2) ln z - z + ln sqrt(2 pi) + s(z),  s(z) = 1/(12 z) - 1/(360 z^3) + 1/(1260 z^5) - 1/(1680 z^7) + 1/(1188 z^9) - ...
    const double z1 = a + 0.5, z0 = a;
    const double r1 = 1.0 / (z1 * z1), r0 = 1.0 / (z0 * z0);
    const double s1 = (1.0 / 12.0 + r1 * (-1.0 / 360.0 + r1 * (1.0 / 1260.0 + r1 * (-1.0 / 1680.0 + r1 * (1.0 / 1188.0 + r1 * (-691.0 / 360360.0)))))) / z1;
    const double s0 = (1.0 / 12.0 + r0 * (-1.0 / 360.0 + r0 * (1.0 / 1260.0 + r0 * (-1.0 / 1680.0 + r0 * (1.0 / 1188.0 + r0 * (-691.0 / 360360.0)))))) / z0;
    // a ln(a + 1/2) - (a - 1/2) ln a - 1/2 = a log1p(1 / (2a)) + ln(a) / 2 - 1/2
    return shift + a * log1p(0.5 / a) + 0.5 * log(a) - 0.5 + (s1 - s0);
}

// I_x(a, b) = x^a y^b / B(a, b) / F with y = 1 - x GIVEN (never formed from x: at df = 10^5 and t = 2.4, 1 - x is 6e-5 and a fraction
// in x alone loses four digits there) and F = b_0 + a_1 / (b_1 + a_2 / (b_2 + ...)),
//   a_m = (a + m - 1)(a + b + m - 1) m (b - m) x^2 / (a + 2m - 1)^2
//   b_m = m + m (b - m) x / (a + 2m - 1) + (a + m)(a y - b x + 1 + m (1 + y)) / (a + 2m + 1)
// (Didonato & Morris 1992, eq. 8.17-8.19).  -> F; *ok = 0: not settled.
// Forward first (modified Lentz) until the convergents stand still, which tells how many terms it takes; the value itself comes
// from the same terms taken from the LAST one inwards: a step of that recurrence damps the errors of the steps before it, where
// the forward product keeps every one.
TS_HD double ts_cf_a(double a, double b, double x, double m) {
    const double den = a + 2.0 * m - 1.0;
    return (a + m - 1.0) * (a + b + m - 1.0) * m * (b - m) * x * x / (den * den);
}
TS_HD double ts_cf_b(double a, double b, double x, double y, double m) {
    const double mid = m > 0.0 ? m * (b - m) * x / (a + 2.0 * m - 1.0) : 0.0;      // (m = 0, a = 1: 0 / 0 as it is written)
    return m + mid + (a + m) * (a * y - b * x + 1.0 + m * (1.0 + y)) / (a + 2.0 * m + 1.0);
}
TS_HD double ts_betacf(double a, double b, double x, double y, int *ok) {
    const double tiny = 1e-300;
    double f = ts_cf_b(a, b, x, y, 0.0);
    if (fabs(f) < tiny) f = tiny;
    double c = f, d = 0.0;
    int n_terms = 0;
    for (int m = 1; m <= TS_CF_MAXIT; ++m) {
        const double am = ts_cf_a(a, b, x, (double)m), bm = ts_cf_b(a, b, x, y, (double)m);
        d = bm + am * d; if (fabs(d) < tiny) d = tiny;
        c = bm + am / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = c * d;
        f *= del;
        if (fabs(del - 1.0) < 4.5e-16) { n_terms = m + 2; break; }      // (two ulps; two terms more go into the value)
    }
    *ok = n_terms > 0;
    if (!n_terms) return f;
    double g = ts_cf_b(a, b, x, y, (double)(n_terms + 1));
    for (int m = n_terms + 1; m >= 1; --m) g = ts_cf_b(a, b, x, y, (double)(m - 1)) + ts_cf_a(a, b, x, (double)m) / g;
    return g;
}

// log10 of the two-sided tail probability of |t| with df degrees of freedom (df >= 1, t finite); *ok as above
TS_HD double ts_log10_p(double df, double t, int *ok) {
    const double ln10 = 2.302585092994045684, ln_sqrt_pi = 0.572364942924700087;
    const double a = 0.5 * df, at = fabs(t);
    *ok = 1;
    if (at == 0.0) return 0.0;
    const double r = (at / df) * at;                                  // t^2 / df; x = df / (df + t^2) = 1 / (1 + r), y = 1 - x
    double ln_x, ln_y, x, y;
    if (r < 1e300) {
        ln_x = -log1p(r); x = 1.0 / (1.0 + r); y = r / (1.0 + r);
        ln_y = r < 1e-300 ? 2.0 * log(at) - log(df) + ln_x : log(r) + ln_x;
    } else {                                                          // (df = 1 reaches 1e-290 at |t| = 6e289 only)
        ln_x = log(df) - 2.0 * log(at); x = exp(ln_x); y = 1.0; ln_y = 0.0;
    }
    const double ln_beta = ln_sqrt_pi - ts_lgamma_half_step(a);       // ln B(a, 1/2)
    const double front = a * ln_x + 0.5 * ln_y - ln_beta;             // ln (x^a y^b / B)
    if (x < (a + 1.0) / (a + 2.5)) return (front - log(ts_betacf(a, 0.5, x, y, ok))) / ln10;
    const double q = exp(front - log(ts_betacf(0.5, a, y, x, ok)));   // I_y(1/2, a)
    return log1p(-q) / ln10;
}

TS_HD double ts_round3(double v) { return rint(v * 1000.0) / 1000.0; }

// could np.round(h, 3) differ from np.round(v, 3) for an h within err of v -- another thousandth, or the other zero ("-0.0")?
// (err >= 0; a NaN anywhere: yes)
TS_HD bool ts_tie_between(double lo_v, double hi_v) {
    const double lo = rint(lo_v * 1000.0), hi = rint(hi_v * 1000.0);
    return !(lo == hi) || __builtin_signbit(lo) != __builtin_signbit(hi);
}
TS_HD bool ts_tie(double v, double err) { return ts_tie_between(v - err, v + err); }

// t of (n, mean, var) and the bound (2) on |host t - device t|; sum_abs = sum |x_i|
TS_HD double ts_t(double n, double mean, double var) { return mean / sqrt(var / n); }
TS_HD double ts_t_bound(double n, double mean, double var, double sum_abs) {
    const double u = 1.1102230246251565e-16;
    const double denom = sqrt(var / n), t = mean / denom;
    const double em = (n + 1.0) * u * (sum_abs / n);
    const double ss = var * (n - 1.0);
    const double e_ss = (n + 3.0) * u + n * em * em / ss;
    return 2.0 * (em / denom + fabs(t) * (0.5 * e_ss + 8.0 * u));
}

// (n, mean, var) -> t and log10 p; the status bits above (t and log10 p are NaN where they are not defined)
TS_HD int ts_stat(double n, double mean, double var, double *t, double *log10_p) {
    const double nan = __builtin_nan("");
    *t = nan; *log10_p = nan;
    if (!(n >= 2.0)) return TS_BAD_N;
    if (!(var > 0.0) || !(var < INFINITY) || !(fabs(mean) < INFINITY)) return TS_ZERO_VAR;
    const double tv = ts_t(n, mean, var);
    if (!(fabs(tv) < INFINITY)) return TS_ZERO_VAR;
    int ok;
    const double l = ts_log10_p(n - 1.0, tv, &ok);
    *t = tv; *log10_p = l;
    if (!ok) return TS_NO_CONVERGENCE;
    if (!(l >= TS_LOG10P_MIN)) return TS_FAR_TAIL;
    return TS_OK;
}

// ---- a column's moments: compensated (two-sum) accumulation, so that what the device adds to (2) does not grow with the depth ----
struct TsSum {                           // s + c: the running sum and what its roundings dropped
    double s = 0.0, c = 0.0;
    TS_HD void add(double v) {
        const double t = s + v, bb = t - s;
        c += (s - (t - bb)) + (v - bb);                               // Knuth's two-sum: exact error of s + v
        s = t;
    }
    TS_HD void merge(const TsSum &o) { add(o.s); c += o.c; }
    TS_HD double value() const { return s + c; }
};

// ---- an entry's two printed values: max_j t_j and sum_j -log10 p_j, each with the interval the host's value lies in ----
#define TS_TIE 16                        // a value within its error bound of a rounding tie of np.round(., 3)
#define TS_MAX_DF 100000.0               // (1) is measured up to here
#define TS_DEEP 32                       // more degrees of freedom than TS_MAX_DF

struct TsSite {
    double max_t = 0.0, max_lo = 0.0, max_hi = 0.0;
    double sum = 0.0, sum_lo = 0.0, sum_hi = 0.0;
    int n_cols = 0, flags = 0;
    // one column: n rows, its mean, centred sum of squares and sum of absolute values
    TS_HD void column(double n, double mean, double ss, double sum_abs) {
        double t = 0.0, l = 0.0;
        const double var = ss / (n - 1.0);
        const int st = n - 1.0 > TS_MAX_DF ? TS_DEEP : ts_stat(n, mean, var, &t, &l);
        if (st) { flags |= st; return; }
        const double e = ts_t_bound(n, mean, var, sum_abs);
        if (!(e < INFINITY)) { flags |= TS_TIE; return; }
        int ok_far, ok_near;
        const double at = fabs(t);
        const double l_far = ts_log10_p(n - 1.0, at + e, &ok_far);                  // <= l <= l_near
        const double l_near = ts_log10_p(n - 1.0, at > e ? at - e : 0.0, &ok_near);
        if (!ok_far || !ok_near) flags |= TS_NO_CONVERGENCE;
        if (!(l_far >= TS_LOG10P_MIN)) flags |= TS_FAR_TAIL;
        if (n_cols == 0) { max_t = t; max_lo = t - e; max_hi = t + e; }
        else {
            max_t = t > max_t ? t : max_t;
            max_lo = t - e > max_lo ? t - e : max_lo;
            max_hi = t + e > max_hi ? t + e : max_hi;
        }
        sum += -l;
        sum_hi += -l_far + TS_FN_BOUND * (l_far < -1.0 ? -l_far : 1.0);
        sum_lo += -l_near - TS_FN_BOUND * (l_near < -1.0 ? -l_near : 1.0);
        ++n_cols;
    }
    // -> the two values as np.round(., 3) gives them; flags: why they cannot be vouched for (0: they can)
    TS_HD int finish(double *v_t, double *v_sum) {
        // the host's own -log10 and its sum of n_cols terms, one after the other: (n_cols + 2) roundings of at most the sum
        const double slack = ((double)n_cols + 2.0) * 2.2204460492503131e-16 * sum_hi;
        if (ts_tie_between(max_lo, max_hi) || ts_tie_between(sum_lo - slack, sum_hi + slack)) flags |= TS_TIE;
        *v_t = ts_round3(max_t);
        *v_sum = ts_round3(sum);
        return flags;
    }
};
