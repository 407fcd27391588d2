// mc_sitecluster.inc -- the rows of every site of ONE sample split in two by their currents, and the split set beside the labels: the
// rows of cluster_sites.cluster_sites made on the GPU from the text of a .diffs file (C ABI: mc_sites_cluster,
// mc_sites_cluster_last_stats, mc_sites_cluster_release; Python: Device.sites_cluster, cluster_sites.cluster_sites_device).  Part of
// the mc_bedcompare.hip unit, included behind mc_curcompare.inc: it runs that file's kn_parse (cu_parse_line), kn_group, kn_claim and
// kn_place as they are -- one file is a comparison whose control text is empty: every line is "native" -- with the unit's key table,
// kp_scan and mc_rowtext.h; its own kernels are kl_*.  The rule itself (distances, tie rule, ARI) is csrc/mc_linkage.h.
//
// The result is the host statement's bytes or a decline (status 1, mc_last_error; the stats name the line).  MC_CMP_DECLINE_HIGH_BYTE,
// _CONTROL, _LONG_LINE, _ROWS, _MEMORY, _TABLE, _NUMBER, _CUR_FIELDS, _CUR_VALUES (fewer than 2 columns: line 0), _CUR_POS as in
// mc_curcompare.inc, and _PRINT for a height mc_rowtext.h does not print (inf, or a positive one outside [1e-29, 1e9): the site's head
// line).  There is no code for a value that is not finite: mc_decimal.h hands out no such value -- it declines inf, nan and exponents
// beyond its range as tokens (_NUMBER), and the host words the ValueError.  A depth is never a decline, and neither is a tie: the
// index rule of lk_before is total.
//
// The steps (L lines, S candidate sites = keys with at least -d rows, R their rows, T their first max_depth rows, c columns):
//   kp_count / kp_scan / kp_starts, kn_parse, kn_group   line starts, the lines, per key the smallest line (atomicMin) and the rows
//                (integer atomicAdd), as for compare_currents
//   kl_select / kp_scan   a line is a candidate's head where it is its key's smallest line and the key has -d rows; the scan over the
//                head flags numbers the candidates in the order of their first rows (no atomic decides an order)
//   kl_sites / kp_scan x 2   per candidate: head line, rows n, the rows that are clustered min(n, max_depth); the buckets' and the
//                vectors' offsets
//   kn_claim / kn_place   rows into their site's bucket in arrival order, then by the rank of their line number: ascending line order
//   kl_vectors   a lane per NUMBER of a row whose rank is below max_depth (the truncation): mc_decimal.h -> row-major vectors
//   kl_prepare   a wave per candidate, 64 rows a round: lk_usable per lane (the flat flag), a ballot compacts the usable rows in order,
//                lk_component -> u (correlation) or the raw row (euclidean), the row's methylated flag; usable rows, kept = usable >= -d
//   kp_scan / kl_list   the kept sites of more than 64 usable rows, in site order
//   kl_link_small<32>, <64>   a WAVE per kept site of up to 32 / of 33 .. 64 usable rows, a lane a row: the distances recomputed from
//                the vectors into a 32 x 33 / 64 x 65 LDS matrix (the pitch is odd: a row-per-lane read of 8-byte words meets every
//                bank pair once; the smaller instance holds a quarter of the LDS and runs four times the waves), the lane's nearest
//                neighbour among the living j > lane in registers.  A merge is one wave-wide argmin on (distance, i) by __shfl_xor
//                -- j is the row's own smallest --, one row update by max, and a new neighbour for the lanes that pointed at a or b
//   kl_link_large<LDS>    a WORKGROUP of 256 per kept site of 65 .. MC_CLU_LDS_ROWS = 141 usable rows: the matrix (141 x 141 doubles) and
//                the per-row state in 163 KB of static LDS
//   kl_link_large<slab>   beyond: a grid of persistent workgroups (at most one a CU), each with a slab of deepest x (deepest | 1) doubles
//                of device memory, counted under MCALLER_CMP_DEVICE_BYTES; the grid is halved until the slabs fit, no slab: _MEMORY.
//                Both: a wave scans a row (coalesced, conflict-free) for its nearest neighbour, only rows that pointed at a merged
//                cluster are scanned again (complete-linkage distances only grow); the argmin is a wave reduction and four words of LDS
//   kl_finish    a lane per site: the counts, lk_ari, np.round(., 3), the mixed decision (lk_mixed)
//   kl_size / kp_scan x 2 / kl_write   the row's and the bed line's length, their places, their bytes; two outputs
// No floating-point atomic anywhere; the integer atomics are sums, minima and maxima.
// Resources (tools/kres.py, gfx950; none spills or uses scratch; kn_parse 44, kn_group 41, kn_claim 10, kn_place 12 VGPRs and the kc_*
// figures of mc_bedcompare.hip's header stand as they were):
//   kl_link_small<32>      31 VGPRs,   8448 bytes of LDS (32 x 33 doubles): 5 waves a SIMD by LDS (19 workgroups of one wave a CU)
//   kl_link_small<64>      35 VGPRs,  33280 bytes of LDS (64 x 65 doubles): 4 workgroups of one wave a CU, 1 wave a SIMD -- LDS sets it
//   kl_link_large<LDS>     40 VGPRs, 162384 bytes of static LDS (the matrix 159048, the per-row state 3336): one workgroup a CU
//   kl_link_large<slab>    64 VGPRs,  23736 bytes of LDS (the per-row state of 1024 rows), 6 waves a SIMD; the matrix is in the slab
//   kl_prepare  46 VGPRs    kl_vectors  40    kl_size  52    kl_write  60 (the digit generation of mc_rowtext.h)    kl_finish  25
//   kl_select   6    kl_sites  12    kl_list  6: no LDS, 8 waves a SIMD, as the four above
// Measured (MI355X, tools/cluster_probe.py, profiles/cluster_probe.json and profiles/cluster_kernel_stats.csv; synthetic `-m A`-like
// rows of six columns, sites of depth 15 .. 60 and four deep ones of 100, 200, 400 and 800 rows, a planted second population at every
// fourth site, --metric correlation --max_depth 1024 --mixed_bed, file to file, medians of 3, files in the page cache):
//   2000 + 4 sites / 6.4 MB    1.66 s -> 0.0122 s (x137 against the host statement on the same box, 0.83 ms a site; the device's rows
//                              and bed equal the host's); kernels 10.0 ms
//   20000 + 4 sites / 63 MB    0.0218 s on the device (kernels 15.2 ms); the host was not timed
//   a run of 2000 + 4 sites, by kernel: kl_link_large<slab> 7.86 ms -- three workgroups, one deep site each, the site of 800 rows about
//   10 us a merge: two round trips to the slab and four barriers a merge, nothing else runs beside them --, kl_link_small<64> 0.44,
//   kl_link_large<LDS> 0.29 (one site of 100 rows), kl_prepare 0.16, kn_parse 0.11, kl_link_small<32> 0.10, kn_place 0.09, kl_finish
//   0.09, kl_write 0.04, kn_group 0.04, kl_vectors 0.03, kl_size 0.03, the seven kp_scan 0.14 together.  The deep sites are the
//   file's critical path; the 2000 wave-linked sites take 0.54 ms.  Not measured: --metric euclidean, other column counts, files
//   that are not in the page cache, a file with many deep sites (where the slab grid fills the CUs).
#include "../mc_linkage.h"

constexpr int KL_LDS_PITCH = MC_CLU_LDS_ROWS | 1;
constexpr int KL_THREADS = 256;

struct CluHead {                             // device-side result block of the kl_* kernels (CurHead serves kn_*; its decline word both)
    long long n_rows, n_trunc, n_large, out_bytes, bed_bytes;
    unsigned long long n_kept, n_mixed, n_small, n_lds, n_slab;
    int deepest, pad;
};

struct CluArgs {
    CurArgs cu;                              // what kn_parse, kn_group, kn_claim and kn_place read; S candidates, cnt1 their rows, off1 their buckets
    CluHead *head;
    int depth, max_depth, metric, mixed;
    double min_minor, min_gap;
    // per candidate
    long long *trunc, *voff;                 // rows that are clustered, where their vectors start (in rows)
    int32_t *usable;
    long long *large_flag, *large_pos;
    int32_t *counts;                         // n_1, n_2, m_1, m_2
    double *heights;                         // h_top, h_sub, np.round(ari, 3)
    uint8_t *is_mixed;
    // per clustered row
    double *V, *U;                           // [T, c]: the values as read, the vectors of the usable rows (compacted per site)
    uint8_t *meth, *label;                   // per usable row
    int32_t *large_list;
    int64_t n_large;
    double *slab;
    int64_t slab_stride;                     // doubles a workgroup
};

__global__ __launch_bounds__(256) void kl_select(CluArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.cu.n_lines) return;
    const uint32_t rep = A.cu.rep[li];
    A.cu.flag[li] = rep != CU_NONE && A.cu.key_first[rep] == (uint32_t)li && (long long)A.cu.key_cnt[rep] >= A.depth;
}

__global__ __launch_bounds__(256) void kl_sites(CluArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.cu.n_lines || A.cu.flag[li] == 0) return;
    const long long s = A.cu.site_of[li];
    if (s < 0 || s >= A.cu.S) return;                                  // (cannot be: the scan counted these lines)
    const uint32_t rep = A.cu.rep[li];
    const long long n = A.cu.key_cnt[rep];
    A.cu.head_line[s] = li;
    A.cu.cnt1[s] = n;
    A.trunc[s] = n < A.max_depth ? n : A.max_depth;
    A.cu.key_site[rep] = (int32_t)s;
}

// a lane per NUMBER of the candidates' rows: value j of the row at bucket place r, where its rank is below max_depth
__global__ __launch_bounds__(256) void kl_vectors(CluArgs A) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = A.cu.c;
    if (v >= A.cu.n_rx * c) return;
    const int64_t r = v / c;
    const int j = (int)(v % c);
    const int64_t li = A.cu.rows[r];
    if (li >= A.cu.n_lines) return;
    const CuRow R = cu_row(A.cu, li);
    if (R.s < 0) return;
    const long long place = r - R.off;
    if (place < 0 || place >= A.trunc[R.s]) return;                    // the truncation: a later row is counted in n and not read
    const TabSpan L = cu_line(A.cu, li);
    const char *t = A.cu.text + A.cu.line_start[li];
    int tb = L.t[3] + 1, k = 0, p = L.t[3] + 1;
    for (; p < L.t[4]; ++p)
        if (t[p] == ',') {
            if (k == j) break;
            ++k; tb = p + 1;
        }
    double d = 0.0;
    if (k != j || !dc_parse(t + tb, p - tb, &d)) line_flag(&A.cu.head->decline, li, MC_CMP_DECLINE_NUMBER);
    A.V[(A.voff[R.s] + place) * c + j] = d;
}

// a wave per candidate: the usable rows, compacted in order
__global__ __launch_bounds__(256) void kl_prepare(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= A.cu.S) return;
    const int c = A.cu.c;
    const long long m = A.trunc[s], at = A.voff[s], bucket = A.cu.off1[s];
    long long base = 0;
    for (long long r0 = 0; r0 < m; r0 += 64) {
        const long long r = r0 + lane;
        double mean = 0.0, sd = 1.0;
        const bool ok = r < m && lk_usable(A.V + (at + r) * c, 1, c, A.metric, &mean, &sd);
        const unsigned long long bal = __ballot(ok);
        if (ok) {
            const long long dst = at + base + __popcll(bal & ((1ull << lane) - 1ull));
            for (int k = 0; k < c; ++k) A.U[dst * c + k] = lk_component(A.V[(at + r) * c + k], mean, sd, A.metric);
            const long long li = A.cu.rows[bucket + r];
            if (li < A.cu.n_lines) {                                   // (always: kn_place put a line here)
                const TabSpan L = cu_line(A.cu, li);
                A.meth[dst] = (int)L.t[5] + 1 < (int)L.t[6] && A.cu.text[A.cu.line_start[li] + L.t[5] + 1] == 'm';
            }
        }
        base += __popcll(bal);
    }
    if (lane != 0) return;
    const int usable = (int)base;
    const bool kept = usable >= A.depth;
    A.usable[s] = usable;
    A.large_flag[s] = kept && usable > MC_CLU_WAVE_ROWS;
    if (!kept) return;
    atomicAdd(usable <= MC_CLU_WAVE_ROWS ? &A.head->n_small : usable <= MC_CLU_LDS_ROWS ? &A.head->n_lds : &A.head->n_slab, 1ull);
    if (usable > A.head->deepest) atomicMax(&A.head->deepest, usable);
}

__global__ __launch_bounds__(256) void kl_list(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.cu.S || A.large_flag[s] == 0) return;
    const long long at = A.large_pos[s];
    if (at >= 0 && at < A.n_large) A.large_list[at] = (int32_t)s;
}

// is the candidate (d1, i1) before (d2, i2)?  i < 0: no candidate.  The j of a row is its own smallest, so (distance, i) decides
__device__ __forceinline__ bool kl_takes(double d1, int i1, double d2, int i2) { return i1 >= 0 && (i2 < 0 || lk_before(d1, i1, 0, d2, i2, 0)); }

// the wave's smallest (d, i) on every lane
__device__ __forceinline__ void kl_wave_argmin(double &d, int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o);
        const int oi = __shfl_xor(i, o);
        if (kl_takes(od, oi, d, i)) { d = od; i = oi; }
    }
}

// ROWS 32: sites of up to 32 usable rows (a quarter of the LDS, four times the waves a CU); ROWS 64: 33 .. 64
template <int ROWS>
__global__ __launch_bounds__(64) void kl_link_small(CluArgs A) {
    constexpr int KL_WAVE_PITCH = ROWS + 1;
    __shared__ double s_M[ROWS * KL_WAVE_PITCH];
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = A.usable[s];
    if (n < A.depth || n < 2 || n > ROWS || (ROWS > 32 && n <= 32)) return;
    const int c = A.cu.c;
    const long long at = A.voff[s];
    const double *U = A.U + at * c;
    const bool mine = lane < n;
    double *row = s_M + lane * KL_WAVE_PITCH;
    if (mine)
        for (int j = 0; j < n; ++j) row[j] = lk_dist(U + (long long)lane * c, U + (long long)j * c, c, A.metric);
    __syncthreads();
    unsigned long long alive = n == 64 ? ~0ull : (1ull << n) - 1ull;   // the clusters, by their smallest row
    int member = lane, nnj = -1;
    double height = 0.0, nnd = 0.0;
    bool need = mine;
    for (int left = n;; --left) {
        if (need) { nnj = -1; nnd = 0.0; }
        for (int j = 1; j < n; ++j) {                                  // (j and alive are the wave's: the living columns alone are read)
            if (!((alive >> j) & 1ull)) continue;
            if (need && j > lane) {
                const double d = row[j];
                if (nnj < 0 || d < nnd) { nnd = d; nnj = j; }
            }
        }
        if (left <= 2) break;
        double h = nnd;
        int a = mine && ((alive >> lane) & 1ull) ? (nnj >= 0 ? lane : -1) : -1;
        kl_wave_argmin(h, a);
        if (a < 0) return;                                             // (cannot be: three clusters live)
        const int b = __shfl(nnj, a);
        alive &= ~(1ull << b);
        if (member == b) member = a;
        if (lane == a) height = h;
        const bool live = mine && ((alive >> lane) & 1ull);
        if (live && lane != a) {
            const double x = row[a], y = row[b], v = x > y ? x : y;
            row[a] = v;
            s_M[a * KL_WAVE_PITCH + lane] = v;
        }
        __syncthreads();
        need = live && (lane == a || nnj == a || nnj == b);
    }
    const int other = __ffsll((unsigned long long)(alive & ~1ull)) - 1;
    if (other < 1 || other >= n) return;                               // (cannot be)
    const double h0 = __shfl(height, 0), h1 = __shfl(height, other);
    if (mine) A.label[at + lane] = member == 0 ? 1 : 2;
    if (lane == 0) {
        A.heights[s * 3 + 0] = s_M[other];
        A.heights[s * 3 + 1] = h0 > h1 ? h0 : h1;
    }
}

template <int CAP>
struct KlState {                             // a workgroup's per-row state (LDS)
    double nnd[CAP], height[CAP];
    int nnj[CAP];
    unsigned long long needmask[(CAP + 63) / 64];
    double r_d[KL_THREADS / 64];
    int r_i[KL_THREADS / 64];
    int other;
    unsigned short member[CAP];
    unsigned char alive[CAP];
};

// one site of n rows (2 <= n <= CAP) by a workgroup of KL_THREADS: the matrix M (pitch P) is the workgroup's, in LDS or in its slab
template <int CAP>
__device__ __forceinline__ void kl_link_block(const CluArgs &A, const int64_t s, const int n, double *M, const long long P, KlState<CAP> &S) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = A.cu.c, words = (n + 63) / 64;
    const long long at = A.voff[s];
    const double *U = A.U + at * c;
    for (int idx = t; idx < n * n; idx += KL_THREADS) {
        const int i = idx / n, j = idx - i * n;
        M[i * P + j] = lk_dist(U + (long long)i * c, U + (long long)j * c, c, A.metric);
    }
    for (int k = t; k < n; k += KL_THREADS) { S.alive[k] = 1; S.member[k] = (unsigned short)k; S.height[k] = 0.0; S.nnj[k] = -1; S.nnd[k] = 0.0; }
    if (t < words) S.needmask[t] = (t + 1) * 64 <= n ? ~0ull : (1ull << (n - t * 64)) - 1ull;
    __syncthreads();
    for (int left = n;; --left) {
        // the rows that need a new nearest neighbour, one after the other round the waves
        int seen = 0;
        for (int w = 0; w < words; ++w) {
            unsigned long long bits = S.needmask[w];
            while (bits) {
                const int k = w * 64 + __ffsll(bits) - 1;
                bits &= bits - 1ull;
                if ((seen++ & 3) != wave) continue;
                double bd = 0.0;
                int bj = -1;
                for (int j = k + 1 + lane; j < n; j += 64)
                    if (S.alive[j]) {
                        const double d = M[k * P + j];
                        if (bj < 0 || d < bd) { bd = d; bj = j; }
                    }
                kl_wave_argmin(bd, bj);
                if (lane == 0) { S.nnd[k] = bd; S.nnj[k] = bj; }
            }
        }
        __syncthreads();
        if (left <= 2) break;
        double h = 0.0;
        int a = -1;
        for (int k = t; k < n; k += KL_THREADS)
            if (S.alive[k] && S.nnj[k] >= 0 && (a < 0 || S.nnd[k] < h)) { h = S.nnd[k]; a = k; }
        kl_wave_argmin(h, a);
        if (lane == 0) { S.r_d[wave] = h; S.r_i[wave] = a; }
        __syncthreads();
        h = S.r_d[0]; a = S.r_i[0];
#pragma unroll
        for (int w = 1; w < KL_THREADS / 64; ++w)
            if (kl_takes(S.r_d[w], S.r_i[w], h, a)) { h = S.r_d[w]; a = S.r_i[w]; }
        if (a < 0) return;                                             // (cannot be: three clusters live; the whole workgroup leaves)
        const int b = S.nnj[a];
        __syncthreads();
        for (int k0 = 0; k0 < n; k0 += KL_THREADS) {
            const int k = k0 + t;
            bool nd = false;
            if (k < n) {
                if (S.member[k] == b) S.member[k] = (unsigned short)a;
                const bool live = S.alive[k] && k != b;
                if (live && k != a) {
                    const double x = M[a * P + k], y = M[b * P + k], v = x > y ? x : y;
                    M[a * P + k] = v;
                    M[k * P + a] = v;
                }
                nd = live && (k == a || S.nnj[k] == a || S.nnj[k] == b);
            }
            const unsigned long long bal = __ballot(nd);
            if (lane == 0 && (k0 >> 6) + wave < words) S.needmask[(k0 >> 6) + wave] = bal;
        }
        if (t == 0) { S.alive[b] = 0; S.height[a] = h; }
        __syncthreads();
    }
    for (int k = t; k < n; k += KL_THREADS) {
        if (k > 0 && S.alive[k]) S.other = k;                          // one row
        A.label[at + k] = S.member[k] == 0 ? 1 : 2;
    }
    __syncthreads();
    if (t == 0) {
        const int other = S.other;
        const double h0 = S.height[0], h1 = S.height[other];
        A.heights[s * 3 + 0] = M[other];
        A.heights[s * 3 + 1] = h0 > h1 ? h0 : h1;
    }
    __syncthreads();
}

// SLAB false: a workgroup per listed site of up to MC_CLU_LDS_ROWS usable rows, the matrix in LDS.  SLAB true: persistent workgroups
// over the listed sites beyond that, the matrix in the workgroup's slab
template <bool SLAB>
__global__ __launch_bounds__(KL_THREADS) void kl_link_large(CluArgs A) {
    constexpr int CAP = SLAB ? MC_CLU_MAX_DEPTH : MC_CLU_LDS_ROWS;
    __shared__ KlState<CAP> s_state;
    __shared__ double s_M[SLAB ? 1 : MC_CLU_LDS_ROWS * KL_LDS_PITCH];
    if (!SLAB) {
        const int64_t s = A.large_list[blockIdx.x];
        const int n = A.usable[s];
        if (n > MC_CLU_WAVE_ROWS && n <= MC_CLU_LDS_ROWS) kl_link_block<CAP>(A, s, n, s_M, KL_LDS_PITCH, s_state);
        return;
    }
    double *M = A.slab + (long long)blockIdx.x * A.slab_stride;
    for (int64_t at = blockIdx.x; at < A.n_large; at += gridDim.x) {
        const int64_t s = A.large_list[at];
        const int n = A.usable[s];
        const long long P = n | 1;
        if (n > MC_CLU_LDS_ROWS && n <= MC_CLU_MAX_DEPTH && (long long)n * P <= A.slab_stride) kl_link_block<CAP>(A, s, n, M, P, s_state);
    }
}

// a lane per candidate: the counts, the adjusted Rand index as it is printed, the mixed decision
__global__ __launch_bounds__(256) void kl_finish(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.cu.S) return;
    A.is_mixed[s] = 0;
    const int n = A.usable[s];
    if (n < A.depth || n < 2) return;
    const long long at = A.voff[s];
    long long n1 = 0, m1 = 0, m2 = 0;
    for (int r = 0; r < n; ++r) {
        const bool first = A.label[at + r] == 1, meth = A.meth[at + r] != 0;
        n1 += first; m1 += first && meth; m2 += !first && meth;
    }
    const long long n2 = n - n1;
    A.counts[s * 4 + 0] = (int32_t)n1; A.counts[s * 4 + 1] = (int32_t)n2; A.counts[s * 4 + 2] = (int32_t)m1; A.counts[s * 4 + 3] = (int32_t)m2;
    if (n1 < 1 || n2 < 1) { line_flag(&A.cu.head->decline, A.cu.head_line[s], MC_CMP_DECLINE_PRINT); return; }      // (cannot be: a link kernel took the site)
    A.heights[s * 3 + 2] = ts_round3(lk_ari(n1, n2, m1, m2));
    A.is_mixed[s] = A.mixed && lk_mixed(n1, n2, A.heights[s * 3 + 0], A.heights[s * 3 + 1], A.min_minor, A.min_gap);
}

template <class Sink>
__device__ __forceinline__ void kl_put_head(const CluArgs &A, const char *p, const TabSpan &L, Sink &o) {
    for (int i = 0; i <= L.t[0]; ++i) o.put(p[i]);                     // chrom and its tab
    for (int i = L.t[1] + 1; i <= L.t[2]; ++i) o.put(p[i]);            // pos
    rt_put_uint(o, cu_pos(p, L) + 1u); o.put('\t');
    for (int i = L.t[2] + 1; i <= L.t[3]; ++i) o.put(p[i]);            // context
}

// chrom pos pos+1 context strand n n_flat n_1 n_2 m_1 m_2 h_top h_sub ari
template <class Sink>
__device__ __forceinline__ void kl_put_row(const CluArgs &A, int64_t s, Sink &o) {
    const long long li = A.cu.head_line[s];
    const TabSpan L = cu_line(A.cu, li);
    const char *p = A.cu.text + A.cu.line_start[li];
    kl_put_head(A, p, L, o);
    for (int i = L.t[4] + 1; i <= L.t[5]; ++i) o.put(p[i]);            // strand
    rt_put_uint(o, (uint32_t)A.cu.cnt1[s]); o.put('\t');
    rt_put_uint(o, (uint32_t)(A.trunc[s] - A.usable[s])); o.put('\t');
    for (int i = 0; i < 4; ++i) { rt_put_uint(o, (uint32_t)A.counts[s * 4 + i]); o.put('\t'); }
    for (int i = 0; i < 3; ++i) { rt_put_num(o, rt_num_of(A.heights[s * 3 + i])); o.put(i < 2 ? '\t' : '\n'); }
}

// chrom pos pos+1 context h_top strand n
template <class Sink>
__device__ __forceinline__ void kl_put_bed(const CluArgs &A, int64_t s, Sink &o) {
    const long long li = A.cu.head_line[s];
    const TabSpan L = cu_line(A.cu, li);
    const char *p = A.cu.text + A.cu.line_start[li];
    kl_put_head(A, p, L, o);
    rt_put_num(o, rt_num_of(A.heights[s * 3 + 0])); o.put('\t');
    for (int i = L.t[4] + 1; i <= L.t[5]; ++i) o.put(p[i]);
    rt_put_uint(o, (uint32_t)A.cu.cnt1[s]); o.put('\n');
}

__global__ __launch_bounds__(256) void kl_size(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool kept = false, mixed = false;
    if (s < A.cu.S) {
        A.cu.row_len[s] = 0; A.cu.bed_len[s] = 0;
        const int n = A.usable[s];
        if (n >= A.depth && n >= 2) {
            bool ok = true;
            for (int i = 0; i < 3; ++i) ok = ok && rt_num_of(A.heights[s * 3 + i]).ok;
            if (!ok) line_flag(&A.cu.head->decline, A.cu.head_line[s], MC_CMP_DECLINE_PRINT);
            else {
                RtCount count;
                kl_put_row(A, s, count);
                A.cu.row_len[s] = count.n;
                kept = true;
                if (A.is_mixed[s]) {
                    RtCount bed;
                    kl_put_bed(A, s, bed);
                    A.cu.bed_len[s] = bed.n;
                    mixed = true;
                }
            }
        }
    }
    const unsigned long long bal = __ballot(kept), bal2 = __ballot(mixed);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_kept, (unsigned long long)__popcll(bal));
    if ((threadIdx.x & 63) == 0 && bal2) atomicAdd(&A.head->n_mixed, (unsigned long long)__popcll(bal2));
}

__global__ __launch_bounds__(256) void kl_write(CluArgs A, char *out, char *bed) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.cu.S) return;
    const long long at = A.cu.row_off[s], len = A.cu.row_len[s];
    if (len > 0 && at >= 0 && at + len <= A.head->out_bytes) {         // (always: the scan counted these bytes)
        RtStore store{out + at};
        kl_put_row(A, s, store);
    }
    const long long bat = A.cu.bed_off[s], blen = A.cu.bed_len[s];
    if (blen > 0 && bat >= 0 && bat + blen <= A.head->bed_bytes) {
        RtStore store{bed + bat};
        kl_put_bed(A, s, store);
    }
}

int clu_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    const char *what = reason == MC_CMP_DECLINE_CUR_VALUES ? "a line whose number of values is not that of the first row, or fewer than 3"
                     : reason == MC_CMP_DECLINE_PRINT ? "a height the device's row writer does not print"
                     : reason == MC_CMP_DECLINE_MEMORY ? "the text, its tables or the distance slabs do not fit into free device memory"
                     : cur_reason_text(reason);
    return decline(c->clu_stats, status, "site clustering", what, reason, line);
}

int clu_decline_head(mc_ctx *c, int32_t *status, const CurHead &h) { return clu_decline(c, status, decline_reason(h.decline), decline_line(h.decline)); }

// The text is on the device (d_text[0, n), padded): everything behind that
int clu_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const mc_clu_options &opt, mc_clu_result *res, int32_t *status) {
    mc_clu_stats &S = c->clu_stats;
    hipStream_t st = c->stream;
    if (n == 0) return 0;
    if (opt.n_columns < 2) return clu_decline(c, status, MC_CMP_DECLINE_CUR_VALUES, 0);
    CurHead *d_cur = nullptr, hc = {};
    CluHead *d_head = nullptr, h = {};
    if (pool.get(&d_cur, 1) || pool.get(&d_head, 1)) return -10;
    hc.decline = CMP_NO_DECLINE;
    HIP_TRY(hipMemcpyAsync(d_cur, &hc, sizeof hc, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, d_text, n, &d_cur->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_cur, hc)) return rc;
    const int64_t n_nl = hc.kp.n_newlines;
    if (too_many_lines(n_nl)) return clu_decline(c, status, MC_CMP_DECLINE_ROWS, -1);
    const size_t cap = (size_t)n_nl + 2;
    if (!cmp_fits(cap * (8 + 16 + 8 + 4 + 4 + 8 + 8 + 4 + 4 + 4) + ((size_t)1 << 20))) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    if (int rc = lines_starts(pool, st, d_text, n, n_nl, tile_off, &d_cur->kp, &line_start)) return rc;
    if (int rc = fetch_head(st, d_cur, hc)) return rc;
    const int64_t L = hc.kp.n_lines;
    if (L <= 0 || L > (int64_t)cap) return 0;
    S.n_lines = L;
    CluArgs A = {};
    CurArgs &Q = A.cu;
    Q.text = d_text; Q.n_bytes = n; Q.off2 = n; Q.n_nl = n_nl; Q.n_lines = L; Q.n_lines1 = L; Q.line_start = line_start; Q.head = d_cur;
    Q.c = opt.n_columns; Q.by = -1; Q.cap = (int64_t)cap;
    A.head = d_head; A.depth = opt.depth; A.max_depth = opt.max_depth; A.metric = opt.metric; A.mixed = opt.mixed != 0;
    A.min_minor = opt.min_minor; A.min_gap = opt.min_gap;
    const char *hm = getenv("MCALLER_CMP_HASH_MASK");
    Q.hash_mask = hm && *hm ? strtoull(hm, nullptr, 16) : ~0ull;      // (tests: long probe chains)
    if (pool.get(&Q.span, cap) || pool.get(&Q.hash, cap) || pool.get(&Q.n_vals, cap) || pool.get(&Q.rep, cap) || pool.get(&Q.flag, cap) ||
        pool.get(&Q.site_of, cap) || pool.get(&Q.key_first, cap) || pool.get(&Q.key_cnt, cap) || pool.get(&Q.key_site, cap))
        return -10;
    hipLaunchKernelGGL(kn_parse, dim3(blocks(L)), dim3(256), CU_STAGE + 16, st, Q);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_cur, hc)) return rc;
    if (hc.decline != CMP_NO_DECLINE) return clu_decline_head(c, status, hc);
    Q.mask = table_slots(L, 64, "MCALLER_CMP_TABLE_SLOTS") - 1;
    S.table_slots = (int64_t)Q.mask + 1;
    if (!cmp_fits((Q.mask + 1) * 8 + ((size_t)1 << 20))) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    if (int rc = table_get(pool, st, &Q.table, Q.mask + 1)) return rc;
    HIP_TRY(hipMemsetAsync(Q.key_first, 0xff, cap * 4, st));
    HIP_TRY(hipMemsetAsync(Q.key_cnt, 0, cap * 4, st));
    HIP_TRY(hipMemsetAsync(Q.key_site, 0xff, cap * 4, st));
    hipLaunchKernelGGL(kn_group, dim3(blocks(L)), dim3(256), 0, st, Q);
    hipLaunchKernelGGL(kl_select, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)Q.flag, L, Q.site_of, &d_cur->n_sites);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_cur, hc)) return rc;
    S.n_keys = (int64_t)hc.n_keys; S.longest_probe = hc.longest_probe;
    if (hc.decline != CMP_NO_DECLINE) return clu_decline_head(c, status, hc);
    const int64_t NS = hc.n_sites;
    S.n_candidates = NS;
    if (NS <= 0) return 0;
    Q.S = NS;
    const size_t ns = (size_t)NS;
    if (!cmp_fits(ns * (10 * 8 + 2 * 4 + 4 + 16 + 24 + 1 + 4) + ((size_t)1 << 20))) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    if (pool.get(&Q.head_line, ns) || pool.get(&Q.cnt1, ns) || pool.get(&Q.off1, ns) || pool.get(&Q.row_len, ns) || pool.get(&Q.row_off, ns) ||
        pool.get(&Q.bed_len, ns) || pool.get(&Q.bed_off, ns) || pool.get(&Q.fill, 2 * ns) || pool.get(&A.trunc, ns) || pool.get(&A.voff, ns) ||
        pool.get(&A.usable, ns) || pool.get(&A.large_flag, ns) || pool.get(&A.large_pos, ns) || pool.get(&A.counts, 4 * ns) ||
        pool.get(&A.heights, 3 * ns) || pool.get(&A.is_mixed, ns) || pool.get(&A.large_list, ns))
        return -10;
    Q.cnt2 = Q.cnt1; Q.off2r = Q.off1;                                 // (no line is a control's)
    HIP_TRY(hipMemsetAsync(Q.fill, 0, 2 * ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.usable, 0, ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.counts, 0, 4 * ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.heights, 0, 3 * ns * 8, st));
    hipLaunchKernelGGL(kl_sites, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)Q.cnt1, NS, Q.off1, &d_head->n_rows);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.trunc, NS, A.voff, &d_head->n_trunc);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    Q.n_rx = h.n_rows; Q.n_ry = 0;
    const size_t nr = (size_t)h.n_rows, nt = (size_t)h.n_trunc, nv = nt * (size_t)Q.c;
    S.n_rows = h.n_rows;
    if (!cmp_fits(nr * 8 + nv * 16 + nt * 2 + ((size_t)1 << 20))) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    if (pool.get(&Q.claimed, nr + 1) || pool.get(&Q.rows, nr + 1) || pool.get(&A.V, nv + 1) || pool.get(&A.U, nv + 1) || pool.get(&A.meth, nt + 1) ||
        pool.get(&A.label, nt + 1))
        return -10;
    HIP_TRY(hipMemsetAsync(Q.claimed, 0xff, (nr + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(Q.rows, 0xff, (nr + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(A.V, 0, (nv + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(A.U, 0, (nv + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(A.meth, 0, nt + 1, st));
    HIP_TRY(hipMemsetAsync(A.label, 0, nt + 1, st));
    hipLaunchKernelGGL(kn_claim, dim3(blocks(L)), dim3(256), 0, st, Q);
    hipLaunchKernelGGL(kn_place, dim3(blocks(L)), dim3(256), 0, st, Q);
    hipLaunchKernelGGL(kl_vectors, dim3(blocks((int64_t)(nr * (size_t)Q.c))), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kl_prepare, dim3((unsigned)((NS + 3) / 4)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.large_flag, NS, A.large_pos, &d_head->n_large);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (int rc = fetch_head(st, d_cur, hc)) return rc;
    if (hc.decline != CMP_NO_DECLINE) return clu_decline_head(c, status, hc);
    S.n_link_small = (int64_t)h.n_small; S.n_link_lds = (int64_t)h.n_lds; S.n_link_slab = (int64_t)h.n_slab; S.deepest_site = h.deepest;
    A.n_large = h.n_large;
    if (h.n_slab > 0) {                                                // the slabs: as many persistent workgroups as fit, one a CU at the most
        const int64_t deep = std::min<int64_t>(h.deepest, MC_CLU_MAX_DEPTH);
        A.slab_stride = deep * (deep | 1);
        int64_t groups = std::min<int64_t>((int64_t)h.n_slab, 256);
        while (groups > 0 && !cmp_fits((size_t)groups * (size_t)A.slab_stride * 8 + ((size_t)1 << 20))) groups /= 2;
        if (groups == 0) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
        if (pool.get(&A.slab, (size_t)groups * (size_t)A.slab_stride)) return -10;
        S.slab_groups = groups; S.slab_bytes = groups * A.slab_stride * 8;
    }
    if (h.n_large > 0) hipLaunchKernelGGL(kl_list, dim3(blocks(NS)), dim3(256), 0, st, A);
    if (h.n_small > 0) {
        hipLaunchKernelGGL(kl_link_small<32>, dim3((unsigned)NS), dim3(64), 0, st, A);
        hipLaunchKernelGGL(kl_link_small<MC_CLU_WAVE_ROWS>, dim3((unsigned)NS), dim3(64), 0, st, A);
    }
    if (h.n_lds > 0) hipLaunchKernelGGL(kl_link_large<false>, dim3((unsigned)h.n_large), dim3(KL_THREADS), 0, st, A);
    if (h.n_slab > 0) hipLaunchKernelGGL(kl_link_large<true>, dim3((unsigned)S.slab_groups), dim3(KL_THREADS), 0, st, A);
    hipLaunchKernelGGL(kl_finish, dim3(blocks(NS)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kl_size, dim3(blocks(NS)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)Q.row_len, NS, Q.row_off, &d_head->out_bytes);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)Q.bed_len, NS, Q.bed_off, &d_head->bed_bytes);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (int rc = fetch_head(st, d_cur, hc)) return rc;
    if (hc.decline != CMP_NO_DECLINE) return clu_decline_head(c, status, hc);
    const size_t ob = (size_t)h.out_bytes, bb = (size_t)h.bed_bytes;
    if (!cmp_fits(ob + bb + ((size_t)1 << 20))) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    char *d_out = nullptr, *d_bed = nullptr;
    if (pool.get(&d_out, ob + 1) || pool.get(&d_bed, bb + 1)) return -10;
    hipLaunchKernelGGL(kl_write, dim3(blocks(NS)), dim3(256), 0, st, A, d_out, d_bed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = cur_fetch(c, c->clu_out, c->clu_out_cap, d_out, ob, &res->out, &res->n_out)) return rc;
    if (int rc = cur_fetch(c, c->clu_bed, c->clu_bed_cap, d_bed, bb, &res->bed, &res->n_bed)) return rc;
    S.ms_d2h = ms_since(t_d2h);
    S.n_out_bytes = (int64_t)ob; S.n_bed_bytes = (int64_t)bb; S.n_sites = (int64_t)h.n_kept; S.n_mixed = (int64_t)h.n_mixed;
    res->n_sites = (int64_t)h.n_kept; res->n_mixed = (int64_t)h.n_mixed;
    return 0;
}

int clu_call(mc_ctx *c, const mc_text_source &src, const mc_clu_options &opt, mc_clu_result *res, int32_t *status) {
    HIP_TRY(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    c->clu_stats = mc_clu_stats();
    c->clu_stats.decline_line = -1;
    c->clu_stats.n_bytes = src.n_bytes; c->clu_stats.n_columns = opt.n_columns;
    *res = mc_clu_result();
    *status = 0;
    if (!cmp_fits((size_t)src.n_bytes + 4096)) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    Pool pool("site clustering");
    TextFeed feed(c, (size_t)32 << 20);
    char *d_text = nullptr;
    if (int rc = feed.put(pool, src, &d_text)) return rc;
    feed.times(c->clu_stats, t0);
    const auto t_kernels = std::chrono::steady_clock::now();
    const int rc = clu_run(c, pool, d_text, src.n_bytes, opt, res, status);
    (void)hipStreamSynchronize(c->stream);                             // (an early return: nothing of the pool is in use when it goes)
    c->clu_stats.ms_kernels = ms_since(t_kernels) - c->clu_stats.ms_d2h;
    if (rc != 0 || *status != 0) *res = mc_clu_result();
    c->clu_stats.ms_total = ms_since(t0);
    return rc;
}
