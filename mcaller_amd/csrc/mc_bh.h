// mc_bh.h -- the operations of the Benjamini-Hochberg adjustment in the log domain that the host build (mc_bh_adjust, mc_format.cpp)
// and the kernels (compare/mc_cmpfdr.inc: mc_bh_adjust_device) share; the definition is compare_genomes.bh_log10:
//
//   L_i = log10 p_i <= 0 of row i (NaN: the row is not tested), m the rows that are not NaN, sorted ascending, rank j = 1 .. m:
//     T_(j) = L_(j) + (log10(m) - log10(j))          Q_(j) = min(0.0, min over k >= j of T_(k))
//   and the printed value np.round(0.0 - Q_i, 3).  Equal L get equal Q whichever way they are sorted (of two equal L the later has
//   the smaller T, and the earlier one's minimum runs over it), so the sort needs no tie rule; min is order-free.
//
// bh_key: a 64-bit key whose unsigned order is the order of the doubles (-inf lowest, -0.0 and 0.0 one key, every NaN the highest
// key of all: the untested rows stand behind the m tested ones).  bh_unkey gives the double back.
//
// The bound on |device Q - host Q|, DERIVED (u = 2^-53).  BH is Lipschitz with constant 1 in the sup norm of the T vector -- a
// minimum of terms moves by no more than the terms do, and two rows that swap ranks because their L differ by less than their bounds
// only exchange terms that close -- so it is the largest |device T - host T|:
//   L:            the column's largest bound on |device L - host L| (the caller's: mc_fisher.h, mc_twosample.h)
//   log10:        m and j are integers <= 2^31, exact in fp64; log10 of them lies in [0, 9.4), where an ulp is at most 2^-49 = 16 u.
//                 NumPy's log10 is within 1 ulp and the device's within 4 (its documented 2, doubled): two logarithms, two builds
//                 -> 2 (16 + 64) u = 160 u
//   subtraction:  |log10 m - log10 j| < 16: at most 8 u a build -> 16 u
//   addition:     |T| <= |L| + 9.4 < 360 with L >= BH_L_MIN = -350 (an L below is no logarithm of an fp64 p and is BH_RANGE):
//                 at most 360 u a build -> 720 u
//   =>  BH_SLACK = 896 u < 1.0e-13, and the bound of every Q of a column is (largest L bound of the column) + BH_SLACK.
// bh_finish rounds and runs mc_tstat.h's tie test with that bound: could a Q within it print another thousandth?
#pragma once
#include "mc_tstat.h"

#define BH_OK 0
#define BH_TIE 1                         // a row's value within the column bound of a rounding tie of np.round(., 3)
#define BH_RANGE 2                       // an L above 0 or below BH_L_MIN, or a bound that is negative or not finite

#define BH_L_MIN (-350.0)
#define BH_SLACK 1.0e-13

TS_HD uint64_t bh_key(double L) {
    if (L != L) return ~0ull;
    union { double d; uint64_t b; } v;
    v.d = L == 0.0 ? 0.0 : L;
    return (v.b >> 63) ? ~v.b : v.b | 0x8000000000000000ull;
}
TS_HD double bh_unkey(uint64_t k) {
    union { double d; uint64_t b; } v;
    if (k == ~0ull) return __builtin_nan("");
    v.b = (k >> 63) ? k & 0x7fffffffffffffffull : ~k;
    return v.d;
}

// could the row be adjusted at all?  (NaN is an untested row: fine)
TS_HD bool bh_in_range(double L, double bound) { return (L != L || (L <= 0.0 && L >= BH_L_MIN)) && bound >= 0.0 && bound < INFINITY; }

// T of rank j (1-based) among m; log10m = log10((double)m)
TS_HD double bh_term(double L, double log10m, long long j) { return L + (log10m - log10((double)j)); }

// Q and the printed value from the minimum of the terms behind a row; BH_TIE when a Q within col_bound + BH_SLACK could print another
// thousandth (0.0 - Q is never below +0.0)
TS_HD int bh_finish(double t_min, double col_bound, double *Q, double *rounded) {
    const double q = t_min < 0.0 ? t_min : 0.0, e = col_bound + BH_SLACK;
    *Q = q;
    *rounded = ts_round3(0.0 - q);
    double lo = (0.0 - q) - e, hi = (0.0 - q) + e;
    if (!(lo > 0.0)) lo = 0.0;
    if (!(hi > 0.0)) hi = 0.0;
    return ts_tie_between(lo, hi) ? BH_TIE : BH_OK;
}
