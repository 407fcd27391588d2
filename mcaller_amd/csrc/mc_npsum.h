// mc_npsum.h -- the three numbers make_bed --gff --vo adds to an entry (make_bed.py:146-149: fracLow, fracUp, identificationQv), in
// NumPy's own order of additions, for a host and a device compiler alike.  C ABI: mc_gff_site_stats, mc_gff_site_moments,
// mc_gff_site_text, mc_npsum_se (the host build, mc_format.cpp), mc_gff_site_stats_device, mc_npsum_se_device (bed/mc_bedsum.hip);
// tests/test_gff_stats.py and tests/test_gpu_bed_gff.py hold both against NumPy.  No kernel is defined here.
//
// Exact by construction: every fp64 operation has the two operands NumPy's has.
//   sum(a)   r = 0.0; for each chunk of NS_CHUNK consecutive elements (the last one shorter): r = r + pw(chunk)
//            (np.add.reduce hands its inner loop at most one buffer's worth of elements at a time)
//   pw(m)    m < 8: 0.0 + a0 + a1 ... left to right
//            8 <= m <= NS_BLOCK: eight accumulators r[j] = a[j]; r[j] += a[i + j] for i = 8, 16, ... < m - m % 8;
//                                ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the m % 8 left-over elements one by one
//            m > NS_BLOCK: h = m / 2, h -= h % 8; pw(first h) + pw(rest)
//   mean     sum(p) / (double)n
//   var      sum((p - mean) * (p - mean)) / (double)(n - 1)      the products rounded before they are summed: no FMA in this unit
//   se       sqrt(var) / sqrt((double)n)                          ns_sqrt: correctly rounded in integers, whatever the library's is
//   fracLow = frac - 2 se, fracUp = frac + 2 se, identificationQv = int(100 * mean), truncated toward zero
// n = 1: var = 0 / 0, the host prints "nan" twice.
//
// A chunk's recursion as a TREE (what a workgroup evaluates: bed/mc_gffstats.inc): node 1 is the chunk, node k has the halves 2k and
// 2k + 1; a node of up to NS_BLOCK elements is a leaf.  A chunk of 8192 elements is seven levels deep at the most (the larger half of
// m elements has at most m / 2 + 7.5: 8192, 4104, 2059, 1037, 526, 270, 143, 79), so NS_NODES = 256 numbers every node.  ns_node
// finds node k's elements from k's bits alone; the host build evaluates the recursion AND the tree and reports a difference.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mc_rowtext.h"

#if defined(__HIP__)
#define NS_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define NS_HD inline
#endif

#define NS_BLOCK 128
#define NS_CHUNK 8192
#define NS_NODES 256

// status bits of ns_finish / mc_gff_site_stats
#define NS_OK 0
#define NS_NAN 1                         // n = 1: fracLow and fracUp are nan (printed as such)
#define NS_PRINT_RANGE 2                 // fracLow or fracUp is a double mc_rowtext.h does not print
#define NS_QV_RANGE 4                    // |100 * mean| >= 2^53, or not finite
#define NS_TREE_MISMATCH 8               // (host build) the tree did not give the recursion's bits
#define NS_BAD_N 16

struct NsPlain {
    const double *a;
    NS_HD double operator()(int64_t i) const { return a[i]; }
};
struct NsSquare {                        // (a[i] - mean)^2, the product rounded
    const double *a;
    double mean;
    NS_HD double operator()(int64_t i) const { const double d = a[i] - mean; return d * d; }
};

// pw of the m <= NS_BLOCK elements g(lo) .. g(lo + m - 1)
template <class G>
NS_HD double ns_leaf(const G &g, int64_t lo, int m) {
    if (m < 8) {
        double r = 0.0;
        for (int i = 0; i < m; ++i) r += g(lo + i);
        return r;
    }
    double r0 = g(lo), r1 = g(lo + 1), r2 = g(lo + 2), r3 = g(lo + 3), r4 = g(lo + 4), r5 = g(lo + 5), r6 = g(lo + 6), r7 = g(lo + 7);
    int i = 8;
    for (; i < m - m % 8; i += 8) {
        r0 += g(lo + i); r1 += g(lo + i + 1); r2 += g(lo + i + 2); r3 += g(lo + i + 3);
        r4 += g(lo + i + 4); r5 += g(lo + i + 5); r6 += g(lo + i + 6); r7 += g(lo + i + 7);
    }
    double r = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < m; ++i) r += g(lo + i);
    return r;
}

// node k (1 <= k < NS_NODES) of the tree of a chunk of m elements -> does it exist; its first element and its length
NS_HD bool ns_node(int m, int k, int *lo, int *len) {
    int a = 0, n = m, depth = 0;
    while ((k >> (depth + 1)) != 0) ++depth;
    for (int b = depth - 1; b >= 0; --b) {
        if (n <= NS_BLOCK) return false;                              // the parent is a leaf
        int h = n / 2;
        h -= h % 8;
        if ((k >> b) & 1) { a += h; n -= h; }
        else n = h;
    }
    *lo = a; *len = n;
    return true;
}

// sqrt(x), correctly rounded: x = f * 2^e with e even and 2^52 <= f < 2^54, F = f * 2^52, R = floor(sqrt(F)) from the library's
// square root put right by integer comparisons; the root lies above R + 1/2 iff F - R^2 > R (it never lies ON it: (R + 1/2)^2 is
// no integer).  Zero, NaN, infinity and negative numbers: the library's answer, which IEEE fixes
NS_HD double ns_sqrt(double x) {
    if (!(x > 0.0) || !(x < INFINITY)) return sqrt(x);
    double scale = 1.0;
    if (x < 2.2250738585072014e-308) { x *= 0x1p108; scale = 0x1p-54; }      // a subnormal: exact both ways
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    uint64_t f = (bits & 0xFFFFFFFFFFFFFull) | (1ull << 52);
    int e = (int)((bits >> 52) & 0x7FF) - 1075;
    if (e & 1) { f <<= 1; e -= 1; }
    const unsigned __int128 F = (unsigned __int128)f << 52;
    uint64_t R = (uint64_t)(sqrt((double)f) * 67108864.0);             // sqrt(F) = sqrt(f) * 2^26, within a few units
    while ((unsigned __int128)R * R > F) --R;
    while ((unsigned __int128)(R + 1) * (R + 1) <= F) ++R;
    if (F - (unsigned __int128)R * R > (unsigned __int128)R) ++R;
    const uint64_t pbits = (uint64_t)((e - 52) / 2 + 1023) << 52;       // 2^((e - 52) / 2): a normal double for every x
    double p;
    __builtin_memcpy(&p, &pbits, 8);
    return (double)R * p * scale;
}

NS_HD double ns_se(double var, double n) { return ns_sqrt(var) / ns_sqrt(n); }

// mean and the sum of the squares -> {fracLow, fracUp, 100 * mean}; the status bits above
NS_HD int ns_finish(double mean, double ss, int64_t n, double frac, double out3[3]) {
    const double var = ss / (double)(n - 1);
    const double se95 = 2.0 * ns_se(var, (double)n);
    out3[0] = frac - se95;
    out3[1] = frac + se95;
    out3[2] = 100.0 * mean;
    int st = NS_OK;
    for (int q = 0; q < 2; ++q) {
        if (!(out3[q] == out3[q])) st |= NS_NAN;
        else if (!rt_num_of(out3[q]).ok) st |= NS_PRINT_RANGE;
    }
    if (!(fabs(out3[2]) < 9007199254740992.0)) st |= NS_QV_RANGE;
    return st;
}

// ";fracLow=<str>;fracUp=<str>;identificationQv=<int>" (lo_nan / hi_nan: "nan"; qv = 100 * mean, |qv| < 2^53, truncated here)
template <class Sink>
NS_HD void ns_put_attributes(Sink &o, const RtNum &lo, bool lo_nan, const RtNum &hi, bool hi_nan, double qv) {
    const char *a = ";fracLow=", *b = ";fracUp=", *c = ";identificationQv=", *nan = "nan";
    for (const char *s = a; *s; ++s) o.put(*s);
    if (lo_nan) for (const char *s = nan; *s; ++s) o.put(*s);
    else rt_put_num(o, lo);
    for (const char *s = b; *s; ++s) o.put(*s);
    if (hi_nan) for (const char *s = nan; *s; ++s) o.put(*s);
    else rt_put_num(o, hi);
    for (const char *s = c; *s; ++s) o.put(*s);
    const int64_t t = (int64_t)qv;                                     // int(): toward zero
    uint64_t m = t < 0 ? (uint64_t)(-t) : (uint64_t)t;
    if (t < 0) o.put('-');
    uint64_t p = 1;
    while (m / p >= 10u) p *= 10u;
    for (; p > 0; p /= 10u) { o.put((char)('0' + m / p)); m %= p; }
}

// ---- the host build (plain host functions): the recursion as NumPy writes it, and the tree as a workgroup evaluates it ----
template <class G>
inline double ns_pw_recursive(const G &g, int64_t lo, int64_t m) {
    if (m <= NS_BLOCK) return ns_leaf(g, lo, (int)m);
    int64_t h = m / 2;
    h -= h % 8;
    return ns_pw_recursive(g, lo, h) + ns_pw_recursive(g, lo + h, m - h);
}

template <class G>
inline double ns_chunk_tree(const G &g, int64_t lo, int m) {
    double val[NS_NODES];
    bool have[NS_NODES];
    for (int k = 1; k < NS_NODES; ++k) {
        int a, n;
        have[k] = ns_node(m, k, &a, &n);
        if (have[k] && n <= NS_BLOCK) val[k] = ns_leaf(g, lo + a, n);
    }
    for (int k = NS_NODES / 2 - 1; k >= 1; --k)
        if (have[k] && have[2 * k]) val[k] = val[2 * k] + val[2 * k + 1];
    return val[1];
}

template <class G>
inline double ns_sum(const G &g, int64_t n, bool tree) {
    double r = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += NS_CHUNK) {
        const int64_t m = n - c0 < NS_CHUNK ? n - c0 : NS_CHUNK;
        r = r + (tree ? ns_chunk_tree(g, c0, (int)m) : ns_pw_recursive(g, c0, m));
    }
    return r;
}

// p[0, n) -> mean, the sum of the squares (and whether the tree gave the same bits)
inline int ns_moments(const double *p, int64_t n, double *mean, double *ss) {
    const NsPlain plain{p};
    const double s = ns_sum(plain, n, false), s_tree = ns_sum(plain, n, true);
    *mean = s / (double)n;
    const NsSquare sq{p, *mean};
    *ss = ns_sum(sq, n, false);
    const double ss_tree = ns_sum(sq, n, true);
    return memcmp(&s, &s_tree, 8) || memcmp(ss, &ss_tree, 8) ? NS_TREE_MISMATCH : NS_OK;
}
