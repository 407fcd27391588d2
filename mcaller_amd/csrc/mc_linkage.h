// mc_linkage.h -- how cluster_sites splits the rows of a site in two (mcaller_amd/cluster_sites.py is the definition), once, for a
// host and a device compiler alike: the two distances, the tie rule, the merge loop over a caller-supplied matrix, the labelling with
// h_top and h_sub, and the adjusted Rand index from four counts.  C ABI: mc_site_cluster_host (the host build, mc_format.cpp; needs
// no GPU), mc_sites_cluster (compare/mc_sitecluster.inc: its link kernels run the merge in parallel -- a lane or a wave per row --
// with lk_dist, lk_before and lk_ari of this header; the serial lk_link below is what they are held against).
// tests/test_cluster_sites.py holds the host build against the Python statement, bit for bit.  No kernel is defined here.
//
// Every operation is fp64 in the order the definition states; the units are built with -ffp-contract=off, sqrt and the division
// are correctly rounded on both sides, max and the comparisons are exact: the device's bits are the host's by construction, and
// nothing here has an error bound.  A complete-linkage distance is a maximum of row distances, so the matrix update
// D(A + B, K) = max(D(A, K), D(B, K)) is the definition's max over all pairs, exactly.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define LK_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define LK_HD inline
#endif

#define LK_CORRELATION 0
#define LK_EUCLIDEAN 1
#define LK_MAX_ROWS 1024                 // --max_depth's cap: the pair counts of lk_ari stay below 2^53

// Is the row v[k * stride] usable -- under correlation: is its centred sum of squares q neither 0 nor not finite (a FLAT row is left
// out), under euclidean: always?  *m the row's mean and *s = sqrt(q) (correlation; 0 and 1 under euclidean)
LK_HD bool lk_usable(const double *v, long long stride, int c, int metric, double *m, double *s) {
    *m = 0.0; *s = 1.0;
    if (metric == LK_EUCLIDEAN) return true;
    double mean = v[0];
    for (int k = 1; k < c; ++k) mean = mean + v[k * stride];
    mean = mean / (double)c;
    double w = v[0] - mean;
    double q = w * w;
    for (int k = 1; k < c; ++k) { w = v[k * stride] - mean; q = q + w * w; }
    if (q == 0.0 || !(q - q == 0.0)) return false;
    *m = mean; *s = sqrt(q);
    return true;
}
// component k of the vector the distance is taken between: u_k under correlation, the value itself under euclidean
LK_HD double lk_component(double v_k, double m, double s, int metric) { return metric == LK_EUCLIDEAN ? v_k : (v_k - m) / s; }

LK_HD bool lk_prepare(const double *v, long long stride, int c, int metric, double *out, long long out_stride) {
    double m, s;
    if (!lk_usable(v, stride, c, metric, &m, &s)) return false;
    for (int k = 0; k < c; ++k) out[k * out_stride] = lk_component(v[k * stride], m, s, metric);
    return true;
}

// d(a, b) between two prepared vectors
LK_HD double lk_dist(const double *a, const double *b, int c, int metric) {
    if (metric == LK_EUCLIDEAN) {
        double e = a[0] - b[0];
        double acc = e * e;
        for (int k = 1; k < c; ++k) { e = a[k] - b[k]; acc = acc + e * e; }
        return sqrt(acc);
    }
    double acc = a[0] * b[0];
    for (int k = 1; k < c; ++k) acc = acc + a[k] * b[k];
    const double d = 1.0 - acc;
    return d > 0.0 ? d : 0.0;                                         // np.maximum(0.0, d): no NaN comes here (|u| <= 1)
}

// The tie rule: is the pair (i1, j1) at distance d1 merged before (i2, j2) at d2?  i the smallest row of the cluster with the smaller
// index, j that of the other: the order is total
LK_HD bool lk_before(double d1, int i1, int j1, double d2, int i2, int j2) {
    if (d1 != d2) return d1 < d2;
    if (i1 != i2) return i1 < i2;
    return j1 < j2;
}

// The merge loop over the square matrix M (M[i * pitch + j], symmetric, n >= 2 rows; it is overwritten) down to two clusters.
// label[i] = 1: row i is in the cluster of row 0, 2: in the other.  A cluster goes by its smallest row.  work: n ints
LK_HD void lk_link(double *M, long long pitch, int n, int *work, uint8_t *label, double *h_top, double *h_sub) {
    int *member = work;
    for (int i = 0; i < n; ++i) { member[i] = i; label[i] = 0; }      // label: 0 while the row's cluster lives under its own number
    // (the height of a cluster -- the distance of its last merge, 0.0 for a singleton -- stands on M's diagonal, which no distance uses)
    for (int i = 0; i < n; ++i) M[i * pitch + i] = 0.0;
    for (int left = n; left > 2; --left) {
        int a = -1, b = -1;
        double d = 0.0;
        for (int i = 0; i < n; ++i) {
            if (member[i] != i) continue;
            for (int j = i + 1; j < n; ++j)
                if (member[j] == j && (a < 0 || lk_before(M[i * pitch + j], i, j, d, a, b))) { a = i; b = j; d = M[i * pitch + j]; }
        }
        for (int k = 0; k < n; ++k) {
            if (member[k] == b) member[k] = a;
            if (k == a || k == b) continue;
            const double x = M[a * pitch + k], y = M[b * pitch + k], v = x > y ? x : y;
            M[a * pitch + k] = v; M[k * pitch + a] = v;
        }
        M[a * pitch + a] = d;
    }
    int other = 1;
    for (int i = n - 1; i > 0; --i) if (member[i] == i) other = i;
    for (int i = 0; i < n; ++i) label[i] = member[i] == 0 ? 1 : 2;
    *h_top = M[other];                                                // row 0
    const double h0 = M[0], h1 = M[other * pitch + other];
    *h_sub = h0 > h1 ? h0 : h1;
}

// The adjusted Rand index of (cluster, methylated): n1, n2 the rows of the two clusters (n1 + n2 <= LK_MAX_ROWS), m1, m2 the
// methylated among them.  Ordered pairs, as sklearn's pair_confusion_matrix counts them
LK_HD double lk_ari(long long n1, long long n2, long long m1, long long m2) {
    const long long n = n1 + n2, u1 = n1 - m1, u2 = n2 - m2;
    const long long ss = m1 * m1 + u1 * u1 + m2 * m2 + u2 * u2;
    const long long tp = ss - n, fp = n1 * n1 + n2 * n2 - ss, fn = (m1 + m2) * (m1 + m2) + (u1 + u2) * (u1 + u2) - ss;
    const long long tn = n * n - fp - fn - ss;
    if (fn == 0 && fp == 0) return 1.0;
    return (double)(2 * (tp * tn - fn * fp)) / (double)((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn));
}

// min(n1, n2) / (n1 + n2) >= min_minor and h_top >= min_gap * h_sub
LK_HD bool lk_mixed(long long n1, long long n2, double h_top, double h_sub, double min_minor, double min_gap) {
    return (double)(n1 < n2 ? n1 : n2) / (double)(n1 + n2) >= min_minor && h_top >= min_gap * h_sub;
}
