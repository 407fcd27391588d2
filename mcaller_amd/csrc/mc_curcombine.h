// mc_curcombine.h -- how compare_currents joins the c value columns of a site into one printed -log10 p per test (Bonferroni over the
// columns, which holds under any dependence between overlapping slots), for a host and a device compiler alike.  C ABI:
// mc_curcombine (the host build, mc_format.cpp; needs no GPU), mc_currents_sites (compare/mc_curcompare.inc: kn_combine, a lane per
// site); tests/test_compare_currents.py holds the host build against the Python statement.  No kernel is defined here.
//
// The statement (compare_currents.py), per test, L_j the unrounded log10 p of column j = 1 .. c:
//     L   = min(0.0, min_j L_j + log10c)          log10c = float(np.log10(c)), handed in as a double: no side calls log10 on c here,
//     nlp = np.round(0.0 - L, 3)                   so the constant is the same bits on both sides
// A NaN among the L_j (SciPy's nan sites) makes L NaN: CC_NAN, nothing is vouched for.
//
// The bound on |device L - host L|, DERIVED (u = 2^-53).  The device's L_j lies within b_j of the host's (tw_finish's bound[5 .. 8]:
// the tail between its two ends and the function terms TW_FN_BOUND / TS_FN_BOUND, measured in profiles/twosample_error.json --
// nothing is measured anew here).
//   minimum:   min is Lipschitz with constant 1 in the sup norm -- the smallest of c numbers moves by no more than the numbers do,
//              whichever column holds it on either side -- so |device min - host min| <= B = max_j b_j.  The minimum itself is
//              exact (a selection, no rounding).
//   sum:       s = fl(min + log10c), ONE rounding on each side, of sums that differ by at most B:
//              |device s - host s| <= B + u |device s| + u |host s| <= B + 2 u (|device s| + B)
//   clamp:     min(0.0, .) is Lipschitz 1 again and exact.
//   =>  bound = B + 2 u (|s| + B).
// The clamp.  Where the device's s is above its bound (s - bound > 0) the host's s is positive too: both sides hold exactly 0.0, the
// bound handed on is 0 and the value is exact for the q-values of mc_bh.h as well.  Where s >= 0 lies within its bound of 0 the device holds
// 0.0 and the host 0.0 or a value above -bound: 0.0 - L is +0.0 or a positive number below 10^-12, both print 0.0 (the tie test
// below sees the interval [0, bound], whose two ends round to +0), so a clamp never declines; the bound goes on to the q-values.
//
// The tie test for three decimals is mc_tstat.h's: with v = 0.0 - L (never below +0.0), could a value within the bound of v print
// another thousandth?  CC_TIE.  The t_j of a row are not combined: each keeps tw_finish's own status.
#pragma once
#include "mc_tstat.h"
#include "mc_rowtext.h"

#define CC_OK 0
#define CC_NAN 1                         // a NaN among the columns' log10 p, or in log10c: the host prints SciPy's nan
#define CC_RANGE 2                       // a column's log10 p above 0 or -inf, a bound that is negative or not finite, c < 1
#define CC_TIE 4                         // the printed value within its bound of a rounding tie of np.round(., 3)
#define CC_UNPRINTABLE 8                 // a value mc_rowtext.h does not print

// the columns of one test, one after the other (any c: nothing is kept but the running minimum and the largest bound)
struct CcMin {
    double m = INFINITY, B = 0.0;
    int flags = 0, n = 0;
    TS_HD void column(double L, double bound) {
        if (L != L) { flags |= CC_NAN; return; }
        if (!(L <= 0.0) || !(L > -INFINITY) || !(bound >= 0.0) || !(bound < INFINITY)) { flags |= CC_RANGE; return; }
        m = L < m ? L : m;
        B = bound > B ? bound : B;
        ++n;
    }
    // -> the status bits; *L the combined log10 p (unrounded, for mc_bh.h), *bound the bound on it, *rounded np.round(0.0 - L, 3)
    TS_HD int finish(double log10c, double *L, double *bound, double *rounded) {
        const double u = 1.1102230246251565e-16, nan = __builtin_nan("");
        *L = nan; *bound = 0.0; *rounded = nan;
        if (log10c != log10c) flags |= CC_NAN;
        if (n < 1 || !(log10c >= 0.0) || !(log10c < INFINITY)) flags |= CC_RANGE;
        if (flags) return flags;
        const double s = m + log10c;
        double e = B + 2.0 * u * (fabs(s) + B);
        double l = s;
        if (s >= 0.0) {
            l = 0.0;
            if (s - e > 0.0) e = 0.0;                                  // clamped on both sides: exact
        }
        const double v = 0.0 - l;
        double lo = v - e, hi = v + e;
        if (!(lo > 0.0)) lo = 0.0;
        if (!(hi > 0.0)) hi = 0.0;
        *L = l; *bound = e; *rounded = ts_round3(v);
        if (ts_tie_between(lo, hi)) flags |= CC_TIE;
        if (!rt_num_of(*rounded).ok) flags |= CC_UNPRINTABLE;
        return flags;
    }
};

// L[0, c) and bound[0, c) at a stride -> as CcMin::finish
TS_HD int cc_combine(const double *L, const double *bound, long long c, long long stride, double log10c, double *out, double *bound_out,
                     double *rounded) {
    CcMin M;
    for (long long j = 0; j < c; ++j) M.column(L[j * stride], bound[j * stride]);
    return M.finish(log10c, out, bound_out, rounded);
}
