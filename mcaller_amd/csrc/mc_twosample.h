// mc_twosample.h -- the two-sample arithmetic of compare_genomes (Mann-Whitney, rank-sum, Student's pooled t, Kolmogorov-Smirnov of
// two samples x[0, n1) and y[0, n2), then np.round(., 3)), for a host and a device compiler alike.  C ABI: mc_twosample (the host
// build, mc_format.cpp), mc_twosample_device (a batch of sites, compare/mc_bedcompare.hip); tests/test_twosample.py and
// tests/test_gpu_compare.py hold both against SciPy.  No kernel is defined here.
//
// What comes in (TwSite) is counted, not rounded: for every pooled value v the four counts #{x < v}, #{x <= v}, #{y < v}, #{y <= v}
// give its midrank (lt + le + 1) / 2 over the pool, its tie-group size t = le - lt and the KS difference at v, so
//   r1x2   = sum over x of (lt + le + 1)            twice the rank sum R1 of x                            (an exact integer)
//   tie    = sum over ALL pooled values of t^2 - 1   = sum over the tie groups of t^3 - t                  (an exact integer)
//   D      = max over v of |#{x <= v} / n1 - #{y <= v} / n2|   two fp64 divisions and a subtraction: ks_2samp's bits
// and the samples' moments: mean_i = (the sum in NumPy's order) / n_i, ss_i = compensated sum of (x - mean_i)^2.
//
//   U1      = R1 - n1 (n1 + 1) / 2                                           exact in fp64 (a multiple of 1/2 below 2^27)
//   z_mwu   = (max(U1, n1 n2 - U1) - n1 n2 / 2 - 1/2) / sqrt(n1 n2 / 12 * ((n + 1) - tie / (n (n - 1))))     mannwhitneyu, asymptotic
//   z_rs    = (R1 - n1 (n + 1) / 2) / sqrt(n1 n2 (n + 1) / 12)                                               ranksums
//   t       = (mean1 - mean2) / sqrt((ss1 + ss2) / (n - 2) * (1 / n1 + 1 / n2))                              ttest_ind, pooled
//   log10 p = log10 erfc(z / sqrt 2) for the two normal tails (min(1, .) for Mann-Whitney: z < 0 there is p = 1),
//             ts_log10_p(n - 2, t) for Student (mc_tstat.h), tw_log10_kolmogorov(sqrt(n1 n2 / n) D) for Smirnov's limit:
//               lam >= 1:  ln Q = ln 2 - 2 lam^2 + log1p(-q^3 + q^8 - q^15 + q^24), q = exp(-2 lam^2)     (the alternating series with
//                          its first term taken out: the logarithm keeps its accuracy where Q is 1e-290)
//               lam <  1:  Q = 1 - sqrt(2 pi) / lam * sum_k exp(-(2k - 1)^2 pi^2 / (8 lam^2)), k = 1 .. 4  (the theta-function form)
//
// The error terms of a printed value (what tw_finish adds up before it asks mc_tstat.h's tie test; a value is exact or declined):
//
// (1) The function terms, MEASURED over the grid of tests/twosample_grid.py (|z| and lam from 1e-6 up to where log10 p reaches
//     TS_LOG10P_MIN; profiles/twosample_error.json, tools/twosample_error.py), host build against SciPy 1.15.3, relative to
//     max(1, |log10 p|):
//         tw_log10_2sf against log10(2 norm.sf(z)):                          3.3e-16   (1125 points; at z 1.31)
//         tw_log10_2sf against (log 2 + norm.logsf(z)) / log 10:             4.4e-16   (at z 3.91)
//         tw_log10_kolmogorov against log10(scipy.special.kolmogorov(lam)):  1.2e-15   (1131 points; at lam 0.84)
//         TW_FN_BOUND (the bound used for both: the largest x 64 = 7.5e-14, rounded up):   8.0e-14
//     The margin covers SciPy's own (unknown) error and the device's erfc / exp / log1p, which are not the host's bit for bit.
//     Student's term is mc_tstat.h's TS_FN_BOUND.
//
// (2) The rank part, DERIVED.  r1x2 and tie are integers below 2^53 (n <= 8192 on the device, 2^20 on the host: tie < n^3), so U1,
//     the two numerators and n1 n2, n (n - 1), n + 1 are exact in fp64 on both sides.  What is left is a handful of roundings:
//         z_rs:   the product's division by 12, the square root, the quotient
//         z_mwu:  n1 n2 / 12, q = tie / (n (n - 1)), d = (n + 1) - q, the product, the square root, the quotient
//     Each is ONE IEEE 754 basic operation (/, -, *, sqrt) on operands that are the same bits on both sides, taken in SciPy's order
//     (tw_finish restates _get_mwu_z and ranksums operation by operation; every unit is built with -ffp-contract=off, so no
//     product is fused into a sum).  Basic operations are correctly rounded on the host and on gfx950 alike, so z_rs and z_mwu are
//     the host's bits: the bound is 0, and an EXACT rounding tie -- z_rs = 13.5 / 72 = 0.1875 where n1 n2 (n + 1) / 12 is a square,
//     one site in 10^4 at depths 15 .. 60 -- rounds half-way to even on both sides instead of declining the file.
//     tests/test_gpu_compare.py prints such a site on the device: a z that differed in its last bit would round the other way.
//
// (3) The moment part, DERIVED.  The two MEANS are NumPy's bits: tw_np_sum adds a sample in np.add.reduce's own order (mc_npsum.h:
//     chunks of 8192, halves down to leaves of 128, eight accumulators), so mean_i = sum / n_i and the numerator mean_1 - mean_2
//     are the host's to the bit.  A site whose means are equal has t = 0.0 on both sides (never -0.0 on one), and the sign of t is
//     the host's everywhere.  The sums of squares are taken about those means: with Q_i = sum (x - mean_i')^2 exactly, the host's
//     ss_i (x - mean rounded, squared, summed pairwise: mc_tstat.h (2)) is Q_i (1 + th_i), |th_i| <= (n_i + 3) u, the device's
//     compensated one is closer, so the pooled SS has the relative error e_ss <= max_i (n_i + 3) u + u (the sum) on either side.
//     denom = sqrt(SS / (n - 2) * (1 / n1 + 1 / n2)): SciPy forms var_i = mean of squares * (n_i / (n_i - 1)), (n_i - 1) var_i, the sum,
//     / df, the two reciprocals and their sum, the product, the square root: ten roundings at the most under the root, which halves
//     them, then the quotient
//      => |t' - t| <= |t| (e_ss / 2 + 8 u)
//     tw_t_bound returns TWICE that.  The bounds on log10 p follow by evaluating the tail at |z| - bound and |z| + bound (each is
//     monotone in |z|); lam = sqrt(n1 n2 / n) D is bit for bit the host's for the reason of (2), 6 u lam is kept as slack.
#pragma once
#include "mc_tstat.h"
#include "mc_rowtext.h"
#include "mc_npsum.h"

#define TW_FN_BOUND 8.0e-14              // see (1)
#define TW_MAX_N 8192                    // pooled values of a site the device ranks (compare/mc_bedcompare.hip: kc_rank_large's LDS)

// status bits of tw_finish (TS_NO_CONVERGENCE = 8 is mc_tstat.h's)
#define TW_OK 0
#define TW_BAD_N 1                       // n1 < 1, n2 < 1 or n < 3: ttest_ind has no degree of freedom, SciPy's nan
#define TW_ZERO_VAR 2                    // the pooled variance is 0 or not finite: SciPy's nan or inf
#define TW_FAR_TAIL 4                    // a log10 p below TS_LOG10P_MIN
#define TW_ALL_EQUAL 16                  // all pooled values equal: the tie-corrected variance is 0, SciPy's nan
#define TW_TIE 32                        // a value within its error bound of a rounding tie of np.round(., 3)
#define TW_UNPRINTABLE 64                // a value mc_rowtext.h does not print
#define TW_DEEP 128                      // more than TW_MAX_N pooled values (the device batch only)

#define TW_N_OUT 9                       // U, z_mwu, z_rs, t, D, nlp_mwu, nlp_rs, nlp_t, nlp_ks: the row's order

struct TwSite {
    long long n1 = 0, n2 = 0;
    long long r1x2 = 0, tie = 0;
    double D = 0.0;
    double mean1 = 0.0, mean2 = 0.0, ss1 = 0.0, ss2 = 0.0;
};

// log10 of 2 sf(z) of the standard normal, z >= 0
TS_HD double tw_log10_2sf(double z) { return log10(erfc(z * 0.70710678118654752440)); }

// log10 of Kolmogorov's Q(lam)
TS_HD double tw_log10_kolmogorov(double lam) {
    const double ln10 = 2.302585092994045684, ln2 = 0.693147180559945309, pi2_8 = 1.2337005501361698274, sqrt_2pi = 2.5066282746310005024;
    if (!(lam > 0.0)) return 0.0;
    if (lam >= 1.0) {
        const double a = 2.0 * lam * lam;
        const double q = exp(-a), q2 = q * q, q3 = q2 * q, q8 = q3 * q3 * q2;
        const double q15 = q8 * q3 * q2 * q2, q24 = q15 * q8 * q;
        return (ln2 - a + log1p(-q3 + q8 - q15 + q24)) / ln10;
    }
    const double w = pi2_8 / (lam * lam);
    if (w > 745.0) return 0.0;                                        // (exp underflows: Q is 1 to the last bit)
    const double s = exp(-w) + exp(-9.0 * w) + exp(-25.0 * w) + exp(-49.0 * w);
    return log1p(-(sqrt_2pi / lam) * s) / ln10;
}

// the bound (3) on |host t - device t|
TS_HD double tw_t_bound(const TwSite &S, double t) {
    const double u = 1.1102230246251565e-16;
    const double n_max = (double)(S.n1 > S.n2 ? S.n1 : S.n2);
    const double e_ss = (n_max + 3.0) * u + u;
    return 2.0 * fabs(t) * (0.5 * e_ss + 8.0 * u);
}

// sum of g(0) .. g(n - 1) in np.add.reduce's order (mc_npsum.h): the recursion of a chunk unrolled over a small stack, for a
// device thread as for the host (a chunk of 8192 is seven levels deep)
template <class G>
TS_HD double tw_np_chunk(const G &g, long long lo, int m) {
    int f_lo[12], f_m[12], f_stage[12], sp = 0;
    double f_left[12], ret = 0.0;
    f_lo[0] = 0; f_m[0] = m; f_stage[0] = 0; f_left[0] = 0.0;
    for (;;) {
        if (f_stage[sp] == 0) {
            if (f_m[sp] <= NS_BLOCK) {
                ret = ns_leaf(g, lo + f_lo[sp], f_m[sp]);
                if (sp == 0) return ret;
                --sp;
                continue;
            }
            int h = f_m[sp] / 2;
            h -= h % 8;
            f_stage[sp] = 1;
            f_lo[sp + 1] = f_lo[sp]; f_m[sp + 1] = h; f_stage[sp + 1] = 0;
            ++sp;
        } else if (f_stage[sp] == 1) {
            int h = f_m[sp] / 2;
            h -= h % 8;
            f_left[sp] = ret;
            f_stage[sp] = 2;
            f_lo[sp + 1] = f_lo[sp] + h; f_m[sp + 1] = f_m[sp] - h; f_stage[sp + 1] = 0;
            ++sp;
        } else {
            ret = f_left[sp] + ret;
            if (sp == 0) return ret;
            --sp;
        }
    }
}
template <class G>
TS_HD double tw_np_sum(const G &g, long long n) {
    if (n <= NS_BLOCK) return 0.0 + ns_leaf(g, 0, (int)n);
    double r = 0.0;
    for (long long c0 = 0; c0 < n; c0 += NS_CHUNK) r = r + tw_np_chunk(g, c0, (int)(n - c0 < NS_CHUNK ? n - c0 : NS_CHUNK));
    return r;
}

// -log10 p of a tail between its two ends l_far <= l <= l_near, with the function term (1): does the printed value stand?
// (the host's value is 0.0 - log10(p) with p <= 1: never below +0.0)
TS_HD bool tw_nlp_tie(double l_far, double l_near, double fn_bound) {
    const double u2 = 2.2204460492503131e-16;
    double hi = -l_far + (fn_bound + 2.0 * u2) * (l_far < -1.0 ? -l_far : 1.0);
    double lo = -l_near - (fn_bound + 2.0 * u2) * (l_near < -1.0 ? -l_near : 1.0);
    if (!(lo > 0.0)) lo = 0.0;
    if (!(hi > 0.0)) hi = 0.0;
    return ts_tie_between(lo, hi);
}

TS_HD double tw_nlp(double log10_p) { return ts_round3(0.0 - log10_p); }

// a site's counts and moments -> the nine values of its row (U and D as they are, the others as np.round(., 3) gives them), the
// bound on |device - host| of each BEFORE rounding (0: exact), and the status bits: why they cannot be vouched for (0: they can)
// logs (null: not wanted): the four log10 p before rounding, in the row's order, for the q-values of mc_bh.h -- bound[5 .. 8] bound them
TS_HD int tw_finish(const TwSite &S, double *out, double *bound, double *logs = nullptr) {
    const double nan = __builtin_nan(""), u = 1.1102230246251565e-16;
    for (int i = 0; i < TW_N_OUT; ++i) { out[i] = nan; bound[i] = 0.0; }
    if (logs) logs[0] = logs[1] = logs[2] = logs[3] = nan;
    if (S.n1 < 1 || S.n2 < 1 || S.n1 + S.n2 < 3) return TW_BAD_N;
    const long long ni = S.n1 + S.n2;
    const double n1 = (double)S.n1, n2 = (double)S.n2, n = (double)ni;
    int flags = 0;
    // ---- ranks ----
    const double R1 = (double)S.r1x2 / 2.0;
    const double U1 = R1 - (double)(S.n1 * (S.n1 + 1)) / 2.0, n1n2 = (double)(S.n1 * S.n2);
    out[0] = U1;
    out[4] = S.D;
    if (S.tie == ni * ni * ni - ni) return TW_ALL_EQUAL | ((S.ss1 + S.ss2 > 0.0) ? 0 : TW_ZERO_VAR);
    const double U2 = n1n2 - U1, U = U1 > U2 ? U1 : U2;
    const double d = (n + 1.0) - (double)S.tie / (double)(ni * (ni - 1));
    const double z_mwu = (U - n1n2 / 2.0 - 0.5) / sqrt(n1n2 / 12.0 * d);
    const double z_rs = (R1 - (double)(S.n1 * (ni + 1)) / 2.0) / sqrt((double)(S.n1 * S.n2 * (ni + 1)) / 12.0);
    const double e_mwu = 0.0, e_rs = 0.0;                             // see (2)
    // ---- moments ----
    const double ss = S.ss1 + S.ss2, df = n - 2.0;
    if (!(ss > 0.0) || !(ss < INFINITY) || !(fabs(S.mean1) < INFINITY) || !(fabs(S.mean2) < INFINITY)) return flags | TW_ZERO_VAR;
    const double denom = sqrt(ss / df * (1.0 / n1 + 1.0 / n2));
    const double t = (S.mean1 - S.mean2) / denom;
    if (!(fabs(t) < INFINITY)) return TW_ZERO_VAR;
    const double e_t = tw_t_bound(S, t);
    if (!(e_t < INFINITY) || !(e_mwu < INFINITY)) flags |= TW_TIE;
    // ---- Smirnov ----
    const double lam = sqrt(n1n2 / n) * S.D, e_lam = 6.0 * u * lam;
    // ---- the four tails, each between its two ends ----
    int ok = 1, ok_far = 1, ok_near = 1;
    const double am = z_mwu > 0.0 ? z_mwu : 0.0, ar = fabs(z_rs), at = fabs(t);
    const double l_mwu = z_mwu > 0.0 ? fmin(0.0, tw_log10_2sf(am)) : 0.0;
    const double l_rs = tw_log10_2sf(ar);
    const double l_t = ts_log10_p(df, t, &ok);
    const double l_ks = tw_log10_kolmogorov(lam);
    const double f_mwu = z_mwu > 0.0 ? fmin(0.0, tw_log10_2sf(am + e_mwu)) : 0.0, n_mwu = am > e_mwu ? fmin(0.0, tw_log10_2sf(am - e_mwu)) : 0.0;
    const double f_rs = tw_log10_2sf(ar + e_rs), n_rs = tw_log10_2sf(ar > e_rs ? ar - e_rs : 0.0);
    const double f_t = ts_log10_p(df, at + e_t, &ok_far), n_t = ts_log10_p(df, at > e_t ? at - e_t : 0.0, &ok_near);
    const double f_ks = tw_log10_kolmogorov(lam + e_lam), n_ks = tw_log10_kolmogorov(lam > e_lam ? lam - e_lam : 0.0);
    if (!ok || !ok_far || !ok_near) flags |= TS_NO_CONVERGENCE;
    if (!(f_mwu >= TS_LOG10P_MIN) || !(f_rs >= TS_LOG10P_MIN) || !(f_t >= TS_LOG10P_MIN) || !(f_ks >= TS_LOG10P_MIN)) flags |= TW_FAR_TAIL;
    if (ts_tie(z_mwu, e_mwu) || ts_tie(z_rs, e_rs) || ts_tie(t, e_t)) flags |= TW_TIE;
    if (tw_nlp_tie(f_mwu, n_mwu, TW_FN_BOUND) || tw_nlp_tie(f_rs, n_rs, TW_FN_BOUND) || tw_nlp_tie(f_t, n_t, TS_FN_BOUND) ||
        tw_nlp_tie(f_ks, n_ks, TW_FN_BOUND))
        flags |= TW_TIE;
    out[1] = ts_round3(z_mwu); out[2] = ts_round3(z_rs); out[3] = ts_round3(t);
    out[5] = tw_nlp(l_mwu); out[6] = tw_nlp(l_rs); out[7] = tw_nlp(l_t); out[8] = tw_nlp(l_ks);
    if (logs) { logs[0] = l_mwu; logs[1] = l_rs; logs[2] = l_t; logs[3] = l_ks; }
    bound[1] = e_mwu; bound[2] = e_rs; bound[3] = e_t;
    bound[5] = (n_mwu - f_mwu) + TW_FN_BOUND * (1.0 - f_mwu); bound[6] = (n_rs - f_rs) + TW_FN_BOUND * (1.0 - f_rs);
    bound[7] = (n_t - f_t) + TS_FN_BOUND * (1.0 - f_t); bound[8] = (n_ks - f_ks) + TW_FN_BOUND * (1.0 - f_ks);
    if (!(flags & TW_FAR_TAIL))
        for (int i = 0; i < TW_N_OUT; ++i)
            if (!rt_num_of(out[i]).ok) flags |= TW_UNPRINTABLE;
    return flags;
}

// ---- a site from its two samples, one value after the other on one thread: the host build's way (mc_twosample) and the statement
// the kernels' counts are held against.  x and y are not changed; O(n^2) comparisons ----
TS_HD void tw_moments(const double *x, long long n, double *mean, double *ss) {
    const NsPlain plain{x};
    const double m = tw_np_sum(plain, n) / (double)n;
    TsSum sq;
    for (long long i = 0; i < n; ++i) { const double d = x[i] - m; sq.add(d * d); }
    *mean = m; *ss = sq.value();
}

// the four counts of v over the two samples -> what v adds to the site
struct TwCount {
    long long r1x2 = 0, tie = 0;
    double D = 0.0;
    TS_HD void value(bool of_x, long long x_lt, long long x_le, long long y_lt, long long y_le, long long n1, long long n2) {
        const long long lt = x_lt + y_lt, le = x_le + y_le, t = le - lt;
        if (of_x) r1x2 += lt + le + 1;
        tie += t * t - 1;
        const double diff = fabs((double)x_le / (double)n1 - (double)y_le / (double)n2);
        D = diff > D ? diff : D;
    }
};
