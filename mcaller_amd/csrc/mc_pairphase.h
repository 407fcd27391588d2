// mc_pairphase.h -- the 2 x 2 table of two sites over the reads that carry a call at both (mcaller_amd/phase_reads.py is the
// definition), once, for a host and a device compiler alike: the four margins, the predicate that says whether the pair is written,
// phi and the three-decimal rounding.  C ABI: mc_pair_phi (the host build, mc_format.cpp; needs no GPU), mc_reads_phase
// (compare/mc_readphase.inc: kr_finish calls pp_written and pp_phi per counter).  tests/test_phase_reads.py holds the host build
// against the Python formula, bit for bit.  No kernel is defined here.
//
//   n11, n10, n01, n00   the shared reads by (A methylated, B methylated); each at most PP_MAX_COUNT = 65535 (a site's depth cap)
//   margins              a1 = n11 + n10, a0 = n01 + n00 (A methylated, not), b1 = n11 + n01, b0 = n10 + n00 (B methylated, not)
//   written              n11 + n10 + n01 + n00 >= min_reads and every margin >= min_margin (>= 1): no written table is degenerate
//   phi                  (double)(n11 n00 - n10 n01) / (sqrt((double)(a1 a0)) * sqrt((double)(b1 b0)))
//
// The integer products are below 2^34 -- exact in 64-bit integers and in fp64 --, the conversions are exact, sqrt and the division
// are correctly rounded on both sides and the units are built with -ffp-contract=off, as for mc_linkage.h: the device's phi has the
// host's bits by construction.  It has no error bound and needs no tie test.  The rounding is mc_tstat.h's ts_round3, which is
// np.round(., 3) for |v| <= 1.
#pragma once
#include "mc_tstat.h"

#define PP_MAX_COUNT 65535LL

struct PpMargins { long long a1, a0, b1, b0; };

TS_HD PpMargins pp_margins(long long n11, long long n10, long long n01, long long n00) { return PpMargins{n11 + n10, n01 + n00, n11 + n01, n10 + n00}; }

TS_HD bool pp_written(long long n11, long long n10, long long n01, long long n00, long long min_reads, long long min_margin) {
    const PpMargins m = pp_margins(n11, n10, n01, n00);
    return n11 + n10 + n01 + n00 >= min_reads && m.a1 >= min_margin && m.a0 >= min_margin && m.b1 >= min_margin && m.b0 >= min_margin;
}

// phi of a table whose four margins are at least 1
TS_HD double pp_phi(long long n11, long long n10, long long n01, long long n00) {
    const PpMargins m = pp_margins(n11, n10, n01, n00);
    const double num = (double)(n11 * n00 - n10 * n01);
    const double den = sqrt((double)(m.a1 * m.a0)) * sqrt((double)(m.b1 * m.b0));
    return num / den;
}

TS_HD double pp_round3(double v) { return ts_round3(v); }
