// mc_sitecluster.inc -- the rows of every site of ONE sample split in two by their currents, and the split set beside the labels: the
// rows of cluster_sites.cluster_sites made on the GPU from the text of a .diffs file (C ABI: mc_sites_cluster,
// mc_sites_cluster_last_stats, mc_sites_cluster_release; Python: Device.sites_cluster, cluster_sites.cluster_sites_device).  Part of
// the mc_bedcompare.hip unit, included behind mc_sitegroup.inc and mc_curcompare.inc: the grouping of the file's lines by site is
// mc_sitegroup.inc's with one file (SgArgs, kn_parse .. kn_place, the host phases of SgRun), the decline texts it shares with the
// comparison are cur_reason_text's; its own kernels are kl_*.  The rule itself (distances, tie rule, ARI) is csrc/mc_linkage.h.
//
// The result is the host statement's bytes or a decline (status 1, mc_last_error; the stats name the line).  MC_CMP_DECLINE_HIGH_BYTE,
// _CONTROL, _LONG_LINE, _ROWS, _MEMORY, _TABLE, _NUMBER, _CUR_FIELDS, _CUR_VALUES (fewer than 2 columns: line 0), _CUR_POS as in
// mc_curcompare.inc, and _PRINT for a height mc_rowtext.h does not print (inf, or a positive one outside [1e-29, 1e9): the site's head
// line).  There is no code for a value that is not finite: mc_decimal.h hands out no such value -- it declines inf, nan and exponents
// beyond its range as tokens (_NUMBER), and the host words the ValueError.  A depth is never a decline, and neither is a tie: the
// index rule of lk_before is total.
//
// The steps (L lines, S candidate sites = keys with at least -d rows, R their rows, T their first max_depth rows, c columns):
//   mc_sitegroup.inc with one file   the line starts, kn_parse, kn_group, kn_select<1>, kn_sites<1>, kn_claim, kn_place: the candidates
//                in the order of their first rows, every candidate's rows in ascending line order
//   kl_trunc / kp_scan   between SgRun::sites and the fetch of the head (one trip for the rows and the clustered rows): per candidate the
//                rows that are clustered min(n, max_depth); the vectors' offsets
//   kl_vectors   a lane per NUMBER of a row whose rank is below max_depth (the truncation): cu_value -> row-major vectors
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
//   kl_size / kp_scan x 2 / kl_write   (sg_outputs) the row's and the bed line's length, their places, their bytes; two outputs
// No floating-point atomic anywhere; the integer atomics are sums, minima and maxima.
// Resources (tools/kres.py, gfx950; none spills or uses scratch; the grouping kernels' figures are in mc_sitegroup.inc's header):
//   kl_link_small<32>      31 VGPRs,   8448 bytes of LDS (32 x 33 doubles): 5 waves a SIMD by LDS (19 workgroups of one wave a CU)
//   kl_link_small<64>      35 VGPRs,  33280 bytes of LDS (64 x 65 doubles): 4 workgroups of one wave a CU, 1 wave a SIMD -- LDS sets it
//   kl_link_large<LDS>     40 VGPRs, 162384 bytes of static LDS (the matrix 159048, the per-row state 3336): one workgroup a CU
//   kl_link_large<slab>    64 VGPRs,  23736 bytes of LDS (the per-row state of 1024 rows), 6 waves a SIMD; the matrix is in the slab
//   kl_prepare  46 VGPRs    kl_vectors  40    kl_size  52    kl_write  60 (the digit generation of mc_rowtext.h)    kl_finish  25
//   kl_trunc    5    kl_list  6: no LDS, 8 waves a SIMD, as the five above
// Measured (MI355X, at the commit that added the pipeline, when it had kl_select and kl_sites of its own; tools/cluster_probe.py,
// profiles/cluster_probe.json and profiles/cluster_kernel_stats.csv; synthetic `-m A`-like rows of six columns, sites of depth 15 .. 60 and four deep ones of 100, 200, 400 and 800 rows, a planted second population at every
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

struct CluHead {                             // device-side result block (copied to the host as it is): grouping's, then the kl_* kernels' own
    SgHead g;                                // n_sites: the candidates, n_rx: their rows
    long long n_trunc, n_large, out_bytes, bed_bytes;
    unsigned long long n_kept, n_mixed, n_small, n_lds, n_slab;
    int deepest, pad;
};

struct CluArgs {
    SgArgs g;                                // the lines, keys, candidates (S; cnt1 their rows, off1 their buckets) and rows of the one file (mc_sitegroup.inc)
    SgOut o;
    CluHead *head;
    int max_depth, metric, mixed;
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

// a lane per candidate: the rows that are clustered
__global__ __launch_bounds__(256) void kl_trunc(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.g.S) return;
    const long long n = A.g.cnt1[s];
    A.trunc[s] = n < A.max_depth ? n : A.max_depth;
}

// a lane per NUMBER of the candidates' rows: value j of the row at bucket place r, where its rank is below max_depth
__global__ __launch_bounds__(256) void kl_vectors(CluArgs A) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = A.g.c;
    if (v >= A.g.n_rx * c) return;
    const int64_t r = v / c;
    const int j = (int)(v % c);
    const int64_t li = A.g.rows[r];
    if (li >= A.g.n_lines) return;
    const CuRow R = cu_row(A.g, li);
    if (R.s < 0) return;
    const long long place = r - R.off;
    if (place < 0 || place >= A.trunc[R.s]) return;                    // the truncation: a later row is counted in n and not read
    A.V[(A.voff[R.s] + place) * c + j] = cu_value(A.g, li, j);
}

// a wave per candidate: the usable rows, compacted in order
__global__ __launch_bounds__(256) void kl_prepare(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= A.g.S) return;
    const int c = A.g.c;
    const long long m = A.trunc[s], at = A.voff[s], bucket = A.g.off1[s];
    long long base = 0;
    for (long long r0 = 0; r0 < m; r0 += 64) {
        const long long r = r0 + lane;
        double mean = 0.0, sd = 1.0;
        const bool ok = r < m && lk_usable(A.V + (at + r) * c, 1, c, A.metric, &mean, &sd);
        const unsigned long long bal = __ballot(ok);
        if (ok) {
            const long long dst = at + base + __popcll(bal & ((1ull << lane) - 1ull));
            for (int k = 0; k < c; ++k) A.U[dst * c + k] = lk_component(A.V[(at + r) * c + k], mean, sd, A.metric);
            const long long li = A.g.rows[bucket + r];
            if (li < A.g.n_lines) {                                   // (always: kn_place put a line here)
                const TabSpan L = cu_line(A.g, li);
                A.meth[dst] = (int)L.t[5] + 1 < (int)L.t[6] && A.g.text[A.g.line_start[li] + L.t[5] + 1] == 'm';
            }
        }
        base += __popcll(bal);
    }
    if (lane != 0) return;
    const int usable = (int)base;
    const bool kept = usable >= A.g.depth;
    A.usable[s] = usable;
    A.large_flag[s] = kept && usable > MC_CLU_WAVE_ROWS;
    if (!kept) return;
    atomicAdd(usable <= MC_CLU_WAVE_ROWS ? &A.head->n_small : usable <= MC_CLU_LDS_ROWS ? &A.head->n_lds : &A.head->n_slab, 1ull);
    if (usable > A.head->deepest) atomicMax(&A.head->deepest, usable);
}

__global__ __launch_bounds__(256) void kl_list(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.g.S || A.large_flag[s] == 0) return;
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
    if (n < A.g.depth || n < 2 || n > ROWS || (ROWS > 32 && n <= 32)) return;
    const int c = A.g.c;
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
    const int c = A.g.c, words = (n + 63) / 64;
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
    if (s >= A.g.S) return;
    A.is_mixed[s] = 0;
    const int n = A.usable[s];
    if (n < A.g.depth || n < 2) return;
    const long long at = A.voff[s];
    long long n1 = 0, m1 = 0, m2 = 0;
    for (int r = 0; r < n; ++r) {
        const bool first = A.label[at + r] == 1, meth = A.meth[at + r] != 0;
        n1 += first; m1 += first && meth; m2 += !first && meth;
    }
    const long long n2 = n - n1;
    A.counts[s * 4 + 0] = (int32_t)n1; A.counts[s * 4 + 1] = (int32_t)n2; A.counts[s * 4 + 2] = (int32_t)m1; A.counts[s * 4 + 3] = (int32_t)m2;
    if (n1 < 1 || n2 < 1) { line_flag(&A.g.head->decline, A.g.head_line[s], MC_CMP_DECLINE_PRINT); return; }      // (cannot be: a link kernel took the site)
    A.heights[s * 3 + 2] = ts_round3(lk_ari(n1, n2, m1, m2));
    A.is_mixed[s] = A.mixed && lk_mixed(n1, n2, A.heights[s * 3 + 0], A.heights[s * 3 + 1], A.min_minor, A.min_gap);
}

// chrom pos pos+1 context strand n n_flat n_1 n_2 m_1 m_2 h_top h_sub ari
template <class Sink>
__device__ __forceinline__ void put_row(const CluArgs &A, int64_t s, Sink &o) {
    const long long li = A.g.head_line[s];
    const TabSpan L = cu_line(A.g, li);
    const char *p = A.g.text + A.g.line_start[li];
    cu_put_prefix(p, L, o);
    cu_put_strand_n(p, L, A.g.cnt1[s], '\t', o);
    rt_put_uint(o, (uint32_t)(A.trunc[s] - A.usable[s])); o.put('\t');
    for (int i = 0; i < 4; ++i) { rt_put_uint(o, (uint32_t)A.counts[s * 4 + i]); o.put('\t'); }
    for (int i = 0; i < 3; ++i) { rt_put_num(o, rt_num_of(A.heights[s * 3 + i])); o.put(i < 2 ? '\t' : '\n'); }
}

__device__ __forceinline__ double bed_value(const CluArgs &A, int64_t s) { return A.heights[s * 3 + 0]; }      // h_top

__global__ __launch_bounds__(256) void kl_size(CluArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool kept = false, mixed = false;
    if (s < A.g.S) {
        A.o.row_len[s] = 0; A.o.bed_len[s] = 0;
        const int n = A.usable[s];
        if (n >= A.g.depth && n >= 2) {
            bool ok = true;
            for (int i = 0; i < 3; ++i) ok = ok && rt_num_of(A.heights[s * 3 + i]).ok;
            if (!ok) line_flag(&A.g.head->decline, A.g.head_line[s], MC_CMP_DECLINE_PRINT);
            else {
                RtCount count;
                put_row(A, s, count);
                A.o.row_len[s] = count.n;
                kept = true;
                if (A.is_mixed[s]) {
                    RtCount bed;
                    cu_put_bed(A.g, s, bed_value(A, s), bed);
                    A.o.bed_len[s] = bed.n;
                    mixed = true;
                }
            }
        }
    }
    const unsigned long long bal = __ballot(kept), bal2 = __ballot(mixed);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_kept, (unsigned long long)__popcll(bal));
    if ((threadIdx.x & 63) == 0 && bal2) atomicAdd(&A.head->n_mixed, (unsigned long long)__popcll(bal2));
}

__global__ __launch_bounds__(256) void kl_write(CluArgs A) { sg_write_site(A); }

int clu_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    const char *what = reason == MC_CMP_DECLINE_CUR_VALUES ? "a line whose number of values is not that of the first row, or fewer than 3"
                     : reason == MC_CMP_DECLINE_PRINT ? "a height the device's row writer does not print"
                     : reason == MC_CMP_DECLINE_MEMORY ? "the text, its tables or the distance slabs do not fit into free device memory"
                     : cur_reason_text(reason);
    return decline(c->clusters.stats, status, "site clustering", what, reason, line);
}

// The text is on the device (d_text[0, n), padded): everything behind that
int clu_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const mc_clu_options &opt, mc_clu_result *res, int32_t *status) {
    mc_clu_stats &S = c->clusters.stats;
    hipStream_t st = c->stream;
    if (n == 0) return 0;
    if (opt.n_columns < 2) return clu_decline(c, status, MC_CMP_DECLINE_CUR_VALUES, 0);
    CluHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    CluArgs A = {};
    SgArgs &G = A.g;
    G.text = d_text; G.n_bytes = n; G.files = 1; G.depth = opt.depth; G.c = opt.n_columns;      // (no pooled_cap: a depth is never a decline)
    A.head = d_head; A.max_depth = opt.max_depth; A.metric = opt.metric; A.mixed = opt.mixed != 0;
    A.min_minor = opt.min_minor; A.min_gap = opt.min_gap;
    SgRun R{pool, st, G, h.g, [&](int reason, long long line) { return clu_decline(c, status, reason, line); }};
    const int rc_keys = R.keys(&d_head->g, sizeof *d_head);
    S.n_lines = R.n_lines; S.table_slots = R.n_slots;
    S.n_keys = (int64_t)h.g.n_keys; S.longest_probe = h.g.longest_probe; S.n_candidates = G.S;
    if (rc_keys) return std::min(rc_keys, 0);
    const int64_t NS = G.S;
    const size_t ns = (size_t)NS;
    // per candidate beside grouping's, as it was charged: the four columns of SgOut and three more, usable, counts, heights, is_mixed, large_list
    if (int rc = R.sites(ns * (7 * 8 + 4 + 16 + 24 + 1 + 4))) return std::min(rc, 0);
    if (pool.get(&A.o.row_len, ns) || pool.get(&A.o.row_off, ns) || pool.get(&A.o.bed_len, ns) || pool.get(&A.o.bed_off, ns) ||
        pool.get(&A.trunc, ns) || pool.get(&A.voff, ns) || pool.get(&A.usable, ns) || pool.get(&A.large_flag, ns) || pool.get(&A.large_pos, ns) ||
        pool.get(&A.counts, 4 * ns) || pool.get(&A.heights, 3 * ns) || pool.get(&A.is_mixed, ns) || pool.get(&A.large_list, ns))
        return -10;
    HIP_TRY(hipMemsetAsync(A.usable, 0, ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.counts, 0, 4 * ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.heights, 0, 3 * ns * 8, st));
    hipLaunchKernelGGL(kl_trunc, dim3(blocks(NS)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.trunc, NS, A.voff, &d_head->n_trunc);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;               // the rows and the clustered rows in one trip
    const size_t nr = (size_t)h.g.n_rx, nt = (size_t)h.n_trunc, nv = nt * (size_t)G.c;
    S.n_rows = h.g.n_rx;
    if (int rc = R.place(nv * 16 + nt * 2)) return std::min(rc, 0);
    if (pool.get(&A.V, nv + 1) || pool.get(&A.U, nv + 1) || pool.get(&A.meth, nt + 1) || pool.get(&A.label, nt + 1)) return -10;
    HIP_TRY(hipMemsetAsync(A.V, 0, (nv + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(A.U, 0, (nv + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(A.meth, 0, nt + 1, st));
    HIP_TRY(hipMemsetAsync(A.label, 0, nt + 1, st));
    hipLaunchKernelGGL(kl_vectors, dim3(blocks((int64_t)(nr * (size_t)G.c))), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kl_prepare, dim3((unsigned)((NS + 3) / 4)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.large_flag, NS, A.large_pos, &d_head->n_large);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.g.decline != CMP_NO_DECLINE) { R.stop_head(); return 0; }
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
    if (int rc = sg_outputs(c, R, A, d_head, h, kl_size, kl_write, c->clusters.out, c->clusters.bed, S, res)) return std::min(rc, 0);
    S.n_sites = (int64_t)h.n_kept; S.n_mixed = (int64_t)h.n_mixed;
    res->n_sites = (int64_t)h.n_kept; res->n_mixed = (int64_t)h.n_mixed;
    return 0;
}

int clu_call(mc_ctx *c, const mc_text_source &src, const mc_clu_options &opt, mc_clu_result *res, int32_t *status) {
    mc_clu_stats &S = c->clusters.stats;
    return pipeline_call(c, S, status, "site clustering", (size_t)32 << 20, [&] { *res = mc_clu_result(); }, [&](Call &K) -> int {
        S.n_bytes = src.n_bytes; S.n_columns = opt.n_columns;
        if (!cmp_fits((size_t)src.n_bytes + 4096)) return clu_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
        char *d_text = nullptr;
        if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;
        K.feed.times(S, K.t0);
        const auto t_kernels = std::chrono::steady_clock::now();
        const int rc = clu_run(c, K.pool, d_text, src.n_bytes, opt, res, status);
        S.ms_kernels = ms_since(t_kernels) - S.ms_d2h;        // a declined call too: what ran until it declined
        return rc;
    });
}
