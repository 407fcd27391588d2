// mc_readphase.inc -- methylation linkage between the sites of ONE sample along its reads: for every pair of kept sites within
// --max_dist the 2 x 2 table of the reads that carry a call at both, phi, Fisher's exact test and its q-value: the rows, the --reads
// rows and the --linked_bed lines of phase_reads.phase_reads made on the GPU from the text of a .diffs file (C ABI: mc_reads_phase,
// mc_reads_phase_last_stats, mc_reads_phase_release; Python: Device.reads_phase, phase_reads.phase_reads_device).  Part of the
// mc_bedcompare.hip unit, included behind mc_sitecluster.inc: the lines, their site keys and the kept sites are mc_sitegroup.inc's
// with one file (SgArgs, kn_parse, kn_group, kn_select<1>, kn_sites<1>: SgRun::keys and ::sites; the site buckets of ::place are
// not needed), the sort is mc_cmpfdr.inc's radix sort, the q-values its fdr_column; the table's arithmetic is csrc/mc_pairphase.h,
// Fisher's mc_fisher.h.  Its own kernels are kr_*.
//
// The result is the host statement's bytes or a decline (status 1, mc_last_error; the stats name the line).  Reused codes:
// MC_CMP_DECLINE_HIGH_BYTE, _CONTROL, _LONG_LINE, _ROWS, _MEMORY, _TABLE (either key table), _NUMBER, _CUR_FIELDS, _CUR_VALUES (no value
// column: line 0), _CUR_POS as in mc_curcompare.inc; _DUPLICATE: a (read key, pos) combination that occurs twice -- the later line
// is named and the host's first-wins rule does the file; _DEPTH: a kept site with more than MC_PHASE_MAX_DEPTH = 65535 rows (its
// head line); _FAR_TAIL, _FISHER_SELECT, _TIE, _PRINT: Fisher's value of a written pair as in kc_fisher_sites (the head line of site
// A), and a q-value within its column's bound of a rounding tie (_TIE, no line).  One new code: MC_CMP_DECLINE_READ_ROWS, a read
// key with more than MC_PHASE_GROUP_ROWS = 2048 rows (its first line).
// Caps: 65535 rows a kept site (the four counts of a pair sit in four 16-bit fields of one word: no field can carry into the next);
// 2048 rows a read key (a workgroup orders them in 16 KB of LDS); S W < 2^31 - 2 counters (_MEMORY); pos of 1 .. 9 plain digits.
//
// The steps (L lines, S kept sites, R read keys, W the widest window, NC = S W counters):
//   SgRun::keys / ::sites   the kept sites numbered in the order of their first rows; per site its head line and rows (N)
//   kr_gclaim / kr_gkey    a lane per kept site: (chrom, strand) into a small key table; the group's smallest head line (atomicMin)
//                names it; the site's sort key is group line << 32 | pos
//   kc_fdr_count / kp_scan / kc_fdr_place   the kept sites sorted once by that key: the genomic rank g of every site.  A site's
//                forward neighbours within max_dist are then g + 1 .. g + w
//   kr_window    a lane per rank: w by a binary search for key + max_dist; W = max w (atomicMax), at least 1; g_of, s_of_g
//   kr_rgroup    a lane per LINE: the hash of (chrom, read, strand) from the spans kn_parse stored, a second key table (kt_claim; the
//                bytes decide, the hash only names the chain); per read key the smallest line (atomicMin) and its rows (atomicAdd)
//   kr_rselect / kp_scan / kr_rsites / kp_scan   the read keys numbered in the order of their first rows; their buckets
//   kr_rclaim    rows into their read's bucket in arrival order
//   kr_order<64, 64> / <256, 2048>   a WAVE per read key of up to 64 rows, a WORKGROUP per read key of up to 2048: a bitonic sort
//                in LDS of pos << 32 | line -- a read's rows share chrom and strand, so pos is their genomic order, and the order
//                is the same whatever the arrival; two neighbours of equal pos are a duplicate.  Per row: pos, the site's g (-1: not
//                kept), methylated, where its read's bucket ends; per read: first, last, calls and methylated calls at kept sites
//   kr_pairs     THE HOT PATH, a lane per row i: it walks the rows j behind it in its read while pos_j - pos_i <= max_dist and
//                makes one 64-bit integer atomicAdd per pair instance into cnt[g_i W + (g_j - g_i - 1)], 1 << 16 (2 (1 - m_i) + (1 - m_j))
//   kr_finish    a lane per counter, site-major (t = s W + k: the order of the rows): the four counts, pp_written, pp_phi, fe_log10p,
//                the status bits and the three-decimal tie test on nlp
//   fdr_column   --fdr: the q-values over all NC counters, the unwritten ones NaN (untested rows stand behind the tested)
//   kr_links     a lane per counter: a written pair whose printed value is at least the threshold adds 1 to both sites (atomicAdd)
//   kr_size<K> / kp_scan / kr_write<K>   K = 0 the rows (a lane per counter), 1 the --reads rows (a lane per read key), 2 the bed
//                (a lane per site): the lengths, the places, the bytes (mc_rowtext.h)
// No floating-point atomic anywhere; the integer atomics are sums, minima and maxima whose results do not depend on arrival, and
// none decides an order or a printed value.
// kr_pairs walks a lane per row.  The other way to spread the walk, a lane per (row, offset), was NOT built and NOT measured: the
// figures below are the lane-per-row walk's alone.
// Resources (tools/kres.py, gfx950; none spills or uses scratch, every one runs at 8 waves a SIMD):
//   kr_finish  58 VGPRs (fe_log10p's two walks)    kr_size<0>  48    kr_write<0>  47 (the digit generation of mc_rowtext.h)
//   kr_rgroup  40    kr_gclaim  36    kr_pairs  24    kr_write<2>  20    kr_size<2>  18    kr_size<1>  15    kr_write<1>  14
//   kr_gkey  14    kr_window  14    kr_links  13    kr_rsites  12    kr_rclaim  10    kr_rselect  6
//   kr_order<64, 64>  16 VGPRs, 528 bytes of LDS    kr_order<256, 2048>  16 VGPRs, 16400 bytes of LDS (2048 keys of 8 bytes)
// Measured (MI355X, at the commit that added the pipeline; tools/phase_probe.py, profiles/phase_probe.json and
// profiles/phase_kernel_stats.csv; synthetic `-m GATC`-like rows of six columns, sites 50 .. 450 bases apart at depth 15 .. 60, reads
// over 10 .. 60 sites, every fourth site driven by one of two planted read populations, --fdr --reads --linked_bed, file to file,
// medians of 3, files in the page cache):
//   2000 sites / 74046 rows / 6.3 MB     0.501 s -> 0.0034 s (x146 against the host statement on the same box; the three files equal
//                                        the host's); kernels 1.54 ms; 242910 pair instances, W = 7, 5551 rows written
//   20000 sites / 747743 rows / 65 MB    5.33 s -> 0.0185 s (x288, files equal); kernels 6.77 ms; 2.5e6 pair instances, W = 8
//   a run of 2000 sites, by kernel: the 23 kp_scan 0.32 ms together (one workgroup each: the largest share), the 15 radix passes 0.20,
//   kn_parse 0.11, kr_rgroup 0.09, kr_rsites 0.07 (every read key adds to one of two counters), kn_group 0.03, kr_gclaim 0.03, kr_pairs
//   0.026, kr_write<0> 0.02, kr_order<64, 64> 0.014, kr_finish 0.011.  At this density the hot path is not where the time goes.
// Not measured: dense `-m A` rows, reads of more than 64 rows (kr_order<256, 2048>), files that are not in the page cache.
#include "../mc_pairphase.h"

constexpr int KR_WAVE_ROWS = MC_PHASE_WAVE_ROWS, KR_GROUP_ROWS = MC_PHASE_GROUP_ROWS;

struct PhHead {                              // device-side result block (copied to the host as it is): grouping's, then the kr_* kernels' own
    SgHead g;
    long long n_readkeys, n_bucket, bytes[3]; // totals of the scans: read keys, their rows, the three outputs
    unsigned long long n_rkeys, n_pairs, n_reads, n_linked, n_wave, n_group, n_instances;
    int W, longest_read, read_probe, pad;
};

struct PhArgs {
    SgArgs g;                                // the lines, the site keys, the kept sites (S; head_line, cnt1)
    PhHead *head;
    int max_dist, min_reads, min_margin, fdr, want_bed, pad;
    double threshold;
    // per line: the read key
    uint32_t *rrep;                          // the line that names the line's read key
    long long *rflag, *read_of;              // 1 at a read key's first line, the scan
    unsigned long long *rtable;
    uint64_t rmask;
    // per read key, at the line that names it
    uint32_t *rk_first, *rk_cnt;
    int32_t *rk_read;
    // per read key, numbered in first-row order
    int64_t R;
    long long *r_head, *r_cnt, *r_off;
    unsigned int *r_fill;
    int32_t *r_stat;                         // [4 R]: first pos, last pos, calls, methylated calls at kept sites
    // per row, in its read's bucket
    int64_t NB;
    uint32_t *b_line, *b_pos, *b_end;
    int32_t *b_g;
    uint8_t *b_m;
    // per kept site
    unsigned long long *gtable;
    uint64_t gmask;
    uint32_t *grp_first;                     // per line: the smallest head line of the (chrom, strand) group the line names
    uint32_t *s_grep;
    unsigned long long *skey;
    uint32_t *srow;
    const unsigned long long *skey_sorted;
    const uint32_t *srow_sorted;
    int32_t *g_of, *s_of_g;
    unsigned int *links;
    // per counter: cnt by (g, k), everything else by t = s W + k
    int64_t W, NC;
    unsigned long long *cnt;
    double *L, *bound, *phi3, *nlp3, *nlq3;
    uint8_t *wr;
    long long *len[3], *off[3];
    char *outp[3];
};

__device__ __forceinline__ const char *kr_text(const PhArgs &A, int64_t li) { return A.g.text + A.g.line_start[li]; }

// (chrom, strand) of lines a and b, byte for byte
__device__ __forceinline__ bool kr_same_group(const PhArgs &A, int64_t a, int64_t b) {
    const TabSpan La = cu_line(A.g, a), Lb = cu_line(A.g, b);
    if (La.t[0] != Lb.t[0] || La.t[5] - La.t[4] != Lb.t[5] - Lb.t[4]) return false;
    const char *pa = kr_text(A, a), *pb = kr_text(A, b);
    return same_bytes(pa, pb, La.t[0]) && same_bytes(pa + La.t[4] + 1, pb + Lb.t[4] + 1, La.t[5] - La.t[4] - 1);
}
// (chrom, read, strand)
__device__ __forceinline__ bool kr_same_read(const PhArgs &A, int64_t a, int64_t b) {
    const TabSpan La = cu_line(A.g, a), Lb = cu_line(A.g, b);
    if (La.t[1] != Lb.t[1]) return false;
    return kr_same_group(A, a, b) && same_bytes(kr_text(A, a) + La.t[0] + 1, kr_text(A, b) + Lb.t[0] + 1, La.t[1] - La.t[0] - 1);
}

__global__ __launch_bounds__(256) void kr_gclaim(PhArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.g.S) return;
    const long long li = A.g.head_line[s];
    const TabSpan L = cu_line(A.g, li);
    const char *p = kr_text(A, li);
    KeyHash H;
    H.span(p, L.t[0]); H.sep(); H.span(p + L.t[4] + 1, L.t[5] - L.t[4] - 1);
    const uint64_t h = H.done(A.g.hash_mask);
    const KtHit hit = kt_claim(A.gtable, A.gmask, h, li, [&](int64_t r) { return r >= 0 && r < A.g.n_lines && kr_same_group(A, li, r); });
    if (hit.slot < 0 || hit.id < 0 || hit.id >= A.g.n_lines) { line_flag(&A.g.head->decline, li, MC_CMP_DECLINE_TABLE); A.s_grep[s] = CU_NONE; return; }
    A.s_grep[s] = (uint32_t)hit.id;
    atomicMin(&A.grp_first[hit.id], (uint32_t)li);
}

__global__ __launch_bounds__(256) void kr_gkey(PhArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.g.S) return;
    const long long li = A.g.head_line[s];
    const uint32_t rep = A.s_grep[s];
    const unsigned long long grp = rep == CU_NONE ? 0xffffffffull : A.grp_first[rep];
    A.skey[s] = (grp << 32) | cu_pos(kr_text(A, li), cu_line(A.g, li));
    A.srow[s] = (uint32_t)s;
}

// a lane per genomic rank: the sites behind it within max_dist
__global__ __launch_bounds__(256) void kr_window(PhArgs A) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= A.g.S) return;
    const uint32_t s = A.srow_sorted[g];
    if (s < A.g.S) { A.g_of[s] = (int32_t)g; A.s_of_g[g] = (int32_t)s; }
    const unsigned long long key = A.skey_sorted[g], pos = key & 0xffffffffull, far = pos + (unsigned long long)A.max_dist;
    const unsigned long long limit = (key & ~0xffffffffull) | (far > 0xffffffffull ? 0xffffffffull : far);
    int64_t lo = g + 1, hi = A.g.S;                                    // the first rank whose key is beyond the limit
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.skey_sorted[mid] <= limit) lo = mid + 1; else hi = mid;
    }
    const int64_t w = lo - 1 - g;
    const int wi = (int)(w > 0x7fffffffll ? 0x7fffffffll : w);
    if (wi > A.head->W) atomicMax(&A.head->W, wi);
}

__global__ __launch_bounds__(256) void kr_rgroup(PhArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.g.n_lines) return;
    A.rrep[li] = CU_NONE;
    const TabSpan L = cu_line(A.g, li);
    if (L.len == 0) return;                                            // (a line kn_parse left out: it has declined the file)
    const char *p = kr_text(A, li);
    KeyHash H;
    H.span(p, L.t[0]); H.sep(); H.span(p + L.t[0] + 1, L.t[1] - L.t[0] - 1); H.sep(); H.span(p + L.t[4] + 1, L.t[5] - L.t[4] - 1);
    const uint64_t h = H.done(A.g.hash_mask);
    const KtHit hit = kt_claim(A.rtable, A.rmask, h, li, [&](int64_t r) { return r >= 0 && r < A.g.n_lines && kr_same_read(A, li, r); });
    if (hit.slot < 0 || hit.id < 0 || hit.id >= A.g.n_lines) { line_flag(&A.g.head->decline, li, MC_CMP_DECLINE_TABLE); return; }
    A.rrep[li] = (uint32_t)hit.id;
    atomicAdd(&A.rk_cnt[hit.id], 1u);
    atomicMin(&A.rk_first[hit.id], (uint32_t)li);
    if (hit.claimed) atomicAdd(&A.head->n_rkeys, 1ull);
    const int looked = (int)(hit.looked > 0x7fffffffull ? 0x7fffffffull : hit.looked);
    if (looked > A.head->read_probe) atomicMax(&A.head->read_probe, looked);
}

__global__ __launch_bounds__(256) void kr_rselect(PhArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.g.n_lines) return;
    const uint32_t rep = A.rrep[li];
    A.rflag[li] = rep != CU_NONE && A.rk_first[rep] == (uint32_t)li ? 1 : 0;
}

__global__ __launch_bounds__(256) void kr_rsites(PhArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.g.n_lines || A.rflag[li] == 0) return;
    const long long r = A.read_of[li];
    if (r < 0 || r >= A.R) return;                                     // (cannot be: the scan counted these lines)
    const uint32_t rep = A.rrep[li];
    const long long n = A.rk_cnt[rep];
    A.r_head[r] = li;
    A.r_cnt[r] = n;
    A.rk_read[rep] = (int32_t)r;
    if (n > KR_GROUP_ROWS) line_flag(&A.g.head->decline, li, MC_CMP_DECLINE_READ_ROWS);
    else atomicAdd(n <= KR_WAVE_ROWS ? &A.head->n_wave : &A.head->n_group, 1ull);
    const int deep = (int)(n > 0x7fffffffll ? 0x7fffffffll : n);
    if (deep > A.head->longest_read) atomicMax(&A.head->longest_read, deep);
}

__global__ __launch_bounds__(256) void kr_rclaim(PhArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.g.n_lines) return;
    const uint32_t rep = A.rrep[li];
    if (rep == CU_NONE) return;
    const long long r = A.rk_read[rep];
    if (r < 0 || r >= A.R) return;
    const long long k = atomicAdd(&A.r_fill[r], 1u);
    if (k < A.r_cnt[r] && A.r_off[r] + k < A.NB) A.b_line[A.r_off[r] + k] = (uint32_t)li;      // (always: the counts are kr_rgroup's)
}

// THREADS 64: the read keys of up to 64 rows, a wave each; THREADS 256: those of 65 .. CAP, a workgroup each
template <int THREADS, int CAP>
__global__ __launch_bounds__(THREADS) void kr_order(PhArgs A) {
    __shared__ unsigned long long s_key[CAP];
    __shared__ int s_stat[4];
    const int64_t r = blockIdx.x;
    const int t = threadIdx.x;
    const long long n = A.r_cnt[r], at = A.r_off[r];
    if (n < 1 || n > CAP || (CAP > KR_WAVE_ROWS && n <= KR_WAVE_ROWS) || at < 0 || at + n > A.NB) return;      // (the whole workgroup)
    int P = 1;
    while (P < n) P <<= 1;
    for (int k = t; k < P; k += THREADS) {
        unsigned long long key = ~0ull;
        if (k < n) {
            const uint32_t li = A.b_line[at + k];
            if (li < A.g.n_lines) key = ((unsigned long long)cu_pos(kr_text(A, li), cu_line(A.g, li)) << 32) | li;
        }
        s_key[k] = key;
    }
    if (t == 0) { s_stat[0] = 0x7fffffff; s_stat[1] = -1; s_stat[2] = 0; s_stat[3] = 0; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int k = t; k < P; k += THREADS) {
                const int partner = k ^ stride;
                if (partner > k) {
                    const unsigned long long a = s_key[k], b = s_key[partner];
                    const bool up = (k & size) == 0;
                    if ((a > b) == up) { s_key[k] = b; s_key[partner] = a; }
                }
            }
            __syncthreads();
        }
    for (int k = t; k < (int)n; k += THREADS) {
        const unsigned long long key = s_key[k];
        if (key == ~0ull) continue;                                    // (cannot be: kr_rclaim filled the bucket)
        const uint32_t li = (uint32_t)key, pos = (uint32_t)(key >> 32);
        if (k > 0 && (uint32_t)(s_key[k - 1] >> 32) == pos) line_flag(&A.g.head->decline, li, MC_CMP_DECLINE_DUPLICATE);
        const CuRow row = cu_row(A.g, li);
        const int g = row.s >= 0 ? A.g_of[row.s] : -1;
        const TabSpan L = cu_line(A.g, li);
        const bool meth = (int)L.t[5] + 1 < (int)L.t[6] && kr_text(A, li)[L.t[5] + 1] == 'm';
        A.b_line[at + k] = li; A.b_pos[at + k] = pos; A.b_g[at + k] = g; A.b_m[at + k] = meth ? 1 : 0;
        A.b_end[at + k] = (uint32_t)(at + n);
        if (g >= 0) {
            atomicMin(&s_stat[0], (int)pos); atomicMax(&s_stat[1], (int)pos);
            atomicAdd(&s_stat[2], 1);
            if (meth) atomicAdd(&s_stat[3], 1);
        }
    }
    __syncthreads();
    if (t < 4) A.r_stat[r * 4 + t] = s_stat[t];
}

// the hot path: a lane per row, the rows behind it in its read within max_dist
__global__ __launch_bounds__(256) void kr_pairs(PhArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long made = 0;
    if (i < A.NB) {
        const int gi = A.b_g[i];
        const int64_t end = A.b_end[i] <= A.NB ? A.b_end[i] : A.NB;
        if (gi >= 0 && gi < A.g.S) {
            const uint32_t pi = A.b_pos[i];
            const int mi = A.b_m[i];
            for (int64_t j = i + 1; j < end; ++j) {
                const uint32_t pj = A.b_pos[j];
                if (pj - pi > (uint32_t)A.max_dist) break;             // (the rows stand by ascending pos)
                const int gj = A.b_g[j];
                const int64_t k = (int64_t)gj - gi - 1;
                if (gj < 0 || pj == pi || k < 0 || k >= A.W) continue; // (a site that is not kept; a duplicate: it has declined the file)
                atomicAdd(&A.cnt[(int64_t)gi * A.W + k], 1ull << (16 * (2 * (1 - mi) + (1 - (int)A.b_m[j]))));
                ++made;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) made += __shfl_xor(made, o);
    if ((threadIdx.x & 63) == 0 && made) atomicAdd(&A.head->n_instances, made);
}

__device__ __forceinline__ int64_t kr_site_b(const PhArgs &A, int64_t t) {
    const int64_t s = t / A.W, g = A.g_of[s] + (t - s * A.W) + 1;
    return g < A.g.S ? (int64_t)A.s_of_g[g] : -1;
}

__global__ __launch_bounds__(256) void kr_finish(PhArgs A) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool written = false;
    if (t < A.NC) {
        const int64_t s = t / A.W, k = t - s * A.W;
        const unsigned long long c = A.cnt[(int64_t)A.g_of[s] * A.W + k];
        const long long n11 = c & 0xffffull, n10 = (c >> 16) & 0xffffull, n01 = (c >> 32) & 0xffffull, n00 = c >> 48;
        double l = __builtin_nan(""), b = 0.0, phi = 0.0;
        written = pp_written(n11, n10, n01, n00, A.min_reads, A.min_margin) && kr_site_b(A, t) >= 0;
        if (written) {
            phi = pp_round3(pp_phi(n11, n10, n01, n00));
            int st;
            fe_log10p(n11, n11 + n10, n01, n01 + n00, &l, &b, &st);
            double lo = -l - b, hi = -l + b;
            if (!(lo > 0.0)) lo = 0.0;
            if (!(hi > 0.0)) hi = 0.0;
            const int reason = (st & (FE_BAD_ARGS | FE_FAR_TAIL)) ? MC_CMP_DECLINE_FAR_TAIL : (st & FE_SELECT) ? MC_CMP_DECLINE_FISHER_SELECT
                             : ts_tie_between(lo, hi) ? MC_CMP_DECLINE_TIE : !rt_num_of(tw_nlp(l)).ok ? MC_CMP_DECLINE_PRINT : 0;
            if (reason) line_flag(&A.g.head->decline, A.g.head_line[s], reason);
        }
        A.wr[t] = written ? 1 : 0;
        A.L[t] = l; A.bound[t] = b; A.phi3[t] = phi; A.nlp3[t] = tw_nlp(l); A.nlq3[t] = __builtin_nan("");
    }
    const unsigned long long bal = __ballot(written);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_pairs, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(256) void kr_links(PhArgs A) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= A.NC || !A.wr[t]) return;
    const double v = A.fdr ? A.nlq3[t] : A.nlp3[t];
    if (!(v >= A.threshold)) return;
    const int64_t sb = kr_site_b(A, t);
    atomicAdd(&A.links[t / A.W], 1u);
    if (sb >= 0) atomicAdd(&A.links[sb], 1u);
}

template <class Sink>
__device__ __forceinline__ void kr_put_span(const char *p, int b, int e, char end, Sink &o) {      // bytes [b, e) and `end`
    for (int i = b; i < e; ++i) o.put(p[i]);
    o.put(end);
}

// K = 0: chrom strand posA posB n n11 n10 n01 n00 phi nlp_fisher [nlq_fisher]
// K = 1: chrom read strand first_pos last_pos n_sites n_meth        K = 2: chrom pos pos+1 context n_links strand N
template <int K, class Sink>
__device__ __forceinline__ void kr_put(const PhArgs &A, int64_t i, Sink &o) {
    if (K == 0) {
        const int64_t s = i / A.W, sb = kr_site_b(A, i);
        const long long la = A.g.head_line[s], lb = A.g.head_line[sb];
        const TabSpan L = cu_line(A.g, la), Lb = cu_line(A.g, lb);
        const char *p = kr_text(A, la), *pb = kr_text(A, lb);
        kr_put_span(p, 0, L.t[0], '\t', o);
        kr_put_span(p, L.t[4] + 1, L.t[5], '\t', o);
        kr_put_span(p, L.t[1] + 1, L.t[2], '\t', o);
        kr_put_span(pb, Lb.t[1] + 1, Lb.t[2], '\t', o);
        const unsigned long long c = A.cnt[(int64_t)A.g_of[s] * A.W + (i - s * A.W)];
        const uint32_t n11 = c & 0xffffu, n10 = (c >> 16) & 0xffffu, n01 = (c >> 32) & 0xffffu, n00 = (uint32_t)(c >> 48);
        rt_put_uint(o, n11 + n10 + n01 + n00); o.put('\t');
        rt_put_uint(o, n11); o.put('\t'); rt_put_uint(o, n10); o.put('\t'); rt_put_uint(o, n01); o.put('\t'); rt_put_uint(o, n00); o.put('\t');
        rt_put_num(o, rt_num_of(A.phi3[i])); o.put('\t');
        rt_put_num(o, rt_num_of(A.nlp3[i]));
        if (A.fdr) { o.put('\t'); rt_put_num(o, rt_num_of(A.nlq3[i])); }
        o.put('\n');
    } else if (K == 1) {
        const long long li = A.r_head[i];
        const TabSpan L = cu_line(A.g, li);
        const char *p = kr_text(A, li);
        kr_put_span(p, 0, L.t[1], '\t', o);                           // chrom, its tab, read
        kr_put_span(p, L.t[4] + 1, L.t[5], '\t', o);
        for (int q = 0; q < 4; ++q) { rt_put_uint(o, (uint32_t)A.r_stat[i * 4 + q]); o.put(q < 3 ? '\t' : '\n'); }
    } else {
        const long long li = A.g.head_line[i];
        const TabSpan L = cu_line(A.g, li);
        const char *p = kr_text(A, li);
        cu_put_prefix(p, L, o);
        rt_put_uint(o, A.links[i]); o.put('\t');
        cu_put_strand_n(p, L, A.g.cnt1[i], '\n', o);
    }
}

template <int K>
__device__ __forceinline__ int64_t kr_items(const PhArgs &A) { return K == 0 ? A.NC : K == 1 ? A.R : A.g.S; }

template <int K>
__global__ __launch_bounds__(256) void kr_size(PhArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool put = false;
    if (i < kr_items<K>(A)) {
        if (K == 0) {
            put = A.wr[i] != 0;
            if (put && !(rt_num_of(A.phi3[i]).ok && rt_num_of(A.nlp3[i]).ok && (!A.fdr || rt_num_of(A.nlq3[i]).ok))) {
                line_flag(&A.g.head->decline, A.g.head_line[i / A.W], MC_CMP_DECLINE_PRINT);
                put = false;
            }
        } else if (K == 1) put = A.r_stat[i * 4 + 2] > 0;
        else put = A.want_bed && A.links[i] > 0;
        long long len = 0;
        if (put) {
            RtCount count;
            kr_put<K>(A, i, count);
            len = count.n;
        }
        A.len[K][i] = len;
    }
    if (K == 0) return;
    const unsigned long long bal = __ballot(put);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(K == 1 ? &A.head->n_reads : &A.head->n_linked, (unsigned long long)__popcll(bal));
}

template <int K>
__global__ __launch_bounds__(256) void kr_write(PhArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= kr_items<K>(A)) return;
    const long long at = A.off[K][i], len = A.len[K][i];
    if (len <= 0 || at < 0 || at + len > A.head->bytes[K]) return;     // (beyond: cannot be, the scan counted these bytes)
    RtStore store{A.outp[K] + at};
    kr_put<K>(A, i, store);
}

int ph_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    const char *what = reason == MC_CMP_DECLINE_CUR_VALUES ? "a line whose number of values is not that of the first row, or fewer than 2"
                     : reason == MC_CMP_DECLINE_DUPLICATE ? "a read with two rows at one position"
                     : reason == MC_CMP_DECLINE_DEPTH ? "a kept site with more than 65535 rows"
                     : reason == MC_CMP_DECLINE_READ_ROWS ? "a read with more than 2048 rows"
                     : reason == MC_CMP_DECLINE_FAR_TAIL ? "a log10 p of Fisher's test below -250"
                     : reason == MC_CMP_DECLINE_MEMORY ? "the text, its tables, the pair counters or the sort buffers do not fit into free device memory"
                     : reason == MC_CMP_DECLINE_TABLE ? "a key table (sites, reads or strands) is full"
                     : reason >= MC_CMP_DECLINE_CUR_FIELDS && reason <= MC_CMP_DECLINE_CUR_POS ? cur_reason_text(reason) : cmp_reason_text(reason);
    return decline(c->phase.stats, status, "read phasing", what, reason, line);
}

// a stable LSD radix sort of (key, row) pairs with mc_cmpfdr.inc's kernels; the keys are group line << 32 | pos: the bytes beyond
// the lines' are the same in every key.  *cur: which of B's two buffers holds the result
int ph_sort_sites(hipStream_t st, const FdrBuf &B, int64_t n, int64_t n_lines, int *cur) {
    const size_t wgs = ((size_t)n + FR_CHUNK - 1) / FR_CHUNK;
    *cur = 0;
    for (int sh = 0; sh < 64; sh += 8) {
        if (sh >= 32 && ((uint64_t)n_lines >> (sh - 32)) == 0) continue;      // (no group line has a bit here)
        hipLaunchKernelGGL(kc_fdr_count, dim3((unsigned)wgs), dim3(256), 0, st, (const unsigned long long *)B.key[*cur], n, sh, B.cnt);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)B.cnt, (int64_t)(256 * wgs), B.off, &B.head->scratch);
        hipLaunchKernelGGL(kc_fdr_place, dim3((unsigned)wgs), dim3(256), 0, st, (const unsigned long long *)B.key[*cur], (const uint32_t *)B.row[*cur], n, sh,
                           (const long long *)B.off, B.key[*cur ^ 1], B.row[*cur ^ 1]);
        HIP_TRY(hipGetLastError());
        *cur ^= 1;
    }
    return 0;
}

template <int K>
int ph_launch_size(hipStream_t st, const PhArgs &A, PhHead *d_head, int64_t n) {
    if (n > 0) hipLaunchKernelGGL(kr_size<K>, dim3(blocks(n)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.len[K], n, A.off[K], &d_head->bytes[K]);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The text is on the device (d_text[0, n), padded): everything behind that
int ph_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const mc_phase_options &opt, mc_phase_result *res, int32_t *status) {
    mc_phase_stats &S = c->phase.stats;
    hipStream_t st = c->stream;
    if (n == 0) return 0;
    if (opt.n_columns < 1) return ph_decline(c, status, MC_CMP_DECLINE_CUR_VALUES, 0);
    PhHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    PhArgs A = {};
    SgArgs &G = A.g;
    G.text = d_text; G.n_bytes = n; G.files = 1; G.depth = opt.depth; G.c = opt.n_columns; G.pooled_cap = MC_PHASE_MAX_DEPTH;
    A.head = d_head; A.max_dist = opt.max_dist; A.min_reads = opt.min_reads; A.min_margin = opt.min_margin; A.fdr = opt.fdr != 0;
    A.want_bed = opt.bed != 0; A.threshold = opt.threshold;
    SgRun R{pool, st, G, h.g, [&](int reason, long long line) { return ph_decline(c, status, reason, line); }};
    const int rc_keys = R.keys(&d_head->g, sizeof *d_head);
    S.n_lines = R.n_lines; S.table_slots = R.n_slots;
    S.n_keys = (int64_t)h.g.n_keys; S.longest_probe = h.g.longest_probe; S.n_sites = G.S; S.deepest_site = h.g.deepest;
    if (rc_keys) return std::min(rc_keys, 0);
    const int64_t NS = G.S, L = G.n_lines;
    const size_t ns = (size_t)NS, nl = (size_t)L + 2;
    // per site beside grouping's: s_grep, skey, srow, g_of, s_of_g, links, the bed's len and off, the sort buffers; the strands' table
    A.gmask = table_slots(NS, 64, "MCALLER_CMP_TABLE_SLOTS") - 1;
    if (int rc = R.sites(ns * (4 + 8 + 4 + 4 + 4 + 4 + 16) + fdr_bytes(NS) + (A.gmask + 1) * 8)) return std::min(rc, 0);
    // per line: rrep, rflag, read_of, rk_first, rk_cnt, rk_read, grp_first, the five bucket columns; per read key (at most a line each): r_head,
    // r_cnt, r_off, r_fill, r_stat, the reads' len and off; the read table
    A.rmask = table_slots(L, 64, "MCALLER_CMP_TABLE_SLOTS") - 1;
    S.read_table_slots = (int64_t)A.rmask + 1;
    if (!cmp_fits(nl * (4 + 8 + 8 + 4 + 4 + 4 + 4 + 17 + 8 + 8 + 8 + 4 + 16 + 16) + (A.rmask + 1) * 8 + ((size_t)1 << 20)))
        { R.stop(MC_CMP_DECLINE_MEMORY); return 0; }
    FdrBuf B;
    if (int rc = fdr_alloc(pool, NS, &B)) return rc;
    A.skey = B.key[0]; A.srow = B.row[0];
    if (pool.get(&A.s_grep, ns) || pool.get(&A.g_of, ns) || pool.get(&A.s_of_g, ns) || pool.get(&A.links, ns) || pool.get(&A.len[2], ns) ||
        pool.get(&A.off[2], ns) || pool.get(&A.grp_first, nl) || pool.get(&A.rrep, nl) || pool.get(&A.rflag, nl) || pool.get(&A.read_of, nl) ||
        pool.get(&A.rk_first, nl) || pool.get(&A.rk_cnt, nl) || pool.get(&A.rk_read, nl))
        return -10;
    if (int rc = table_get(pool, st, &A.gtable, A.gmask + 1)) return rc;
    if (int rc = table_get(pool, st, &A.rtable, A.rmask + 1)) return rc;
    HIP_TRY(hipMemsetAsync(A.grp_first, 0xff, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.rk_first, 0xff, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.rk_cnt, 0, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.rk_read, 0xff, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.g_of, 0, ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.s_of_g, 0, ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.links, 0, ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.len[2], 0, ns * 8, st));
    // the kept sites in genomic order
    hipLaunchKernelGGL(kr_gclaim, dim3(blocks(NS)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kr_gkey, dim3(blocks(NS)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    int cur = 0;
    if (int rc = ph_sort_sites(st, B, NS, L, &cur)) return rc;
    A.skey_sorted = B.key[cur]; A.srow_sorted = B.row[cur];
    hipLaunchKernelGGL(kr_window, dim3(blocks(NS)), dim3(256), 0, st, A);
    // the read keys
    hipLaunchKernelGGL(kr_rgroup, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kr_rselect, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.rflag, L, A.read_of, &d_head->n_readkeys);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_read_keys = (int64_t)h.n_rkeys; S.longest_read_probe = h.read_probe;
    if (h.g.decline != CMP_NO_DECLINE) { R.stop_head(); return 0; }
    const int64_t NR = h.n_readkeys;
    if (NR <= 0 || NR > L) return 0;                                   // (cannot be: every line has a read key)
    const size_t nr = (size_t)NR;
    A.R = NR; A.NB = L;
    A.W = std::max<int64_t>(h.W, 1);
    A.NC = NS * A.W;
    S.window = A.W; S.n_counters = A.NC;
    if (pool.get(&A.r_head, nr) || pool.get(&A.r_cnt, nr) || pool.get(&A.r_off, nr) || pool.get(&A.r_fill, nr) || pool.get(&A.r_stat, 4 * nr) ||
        pool.get(&A.len[1], nr) || pool.get(&A.off[1], nr) || pool.get(&A.b_line, nl) || pool.get(&A.b_pos, nl) || pool.get(&A.b_end, nl) ||
        pool.get(&A.b_g, nl) || pool.get(&A.b_m, nl))
        return -10;
    HIP_TRY(hipMemsetAsync(A.r_cnt, 0, nr * 8, st));
    HIP_TRY(hipMemsetAsync(A.r_fill, 0, nr * 4, st));
    HIP_TRY(hipMemsetAsync(A.r_stat, 0, 4 * nr * 4, st));
    HIP_TRY(hipMemsetAsync(A.len[1], 0, nr * 8, st));
    HIP_TRY(hipMemsetAsync(A.b_line, 0xff, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.b_pos, 0, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.b_end, 0, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.b_g, 0xff, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.b_m, 0, nl, st));
    hipLaunchKernelGGL(kr_rsites, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.r_cnt, NR, A.r_off, &d_head->n_bucket);
    hipLaunchKernelGGL(kr_rclaim, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL((kr_order<64, KR_WAVE_ROWS>), dim3((unsigned)NR), dim3(64), 0, st, A);
    hipLaunchKernelGGL((kr_order<256, KR_GROUP_ROWS>), dim3((unsigned)NR), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_reads_wave = (int64_t)h.n_wave; S.n_reads_group = (int64_t)h.n_group; S.longest_read = h.longest_read;
    if (h.g.decline != CMP_NO_DECLINE) { R.stop_head(); return 0; }
    // the counters: cnt, L, bound, phi3, nlp3, nlq3, wr, the rows' len and off; the q-values' sort buffers
    if (A.NC >= ((int64_t)1 << 31) - 2) { R.stop(MC_CMP_DECLINE_MEMORY); return 0; }
    const size_t nc = (size_t)A.NC;
    if (!cmp_fits(nc * (8 + 5 * 8 + 1 + 16) + (A.fdr ? fdr_bytes(A.NC) : 0) + ((size_t)1 << 20))) { R.stop(MC_CMP_DECLINE_MEMORY); return 0; }
    if (pool.get(&A.cnt, nc) || pool.get(&A.L, nc) || pool.get(&A.bound, nc) || pool.get(&A.phi3, nc) || pool.get(&A.nlp3, nc) ||
        pool.get(&A.nlq3, nc) || pool.get(&A.wr, nc) || pool.get(&A.len[0], nc) || pool.get(&A.off[0], nc))
        return -10;
    HIP_TRY(hipMemsetAsync(A.cnt, 0, nc * 8, st));
    HIP_TRY(hipMemsetAsync(A.len[0], 0, nc * 8, st));
    hipLaunchKernelGGL(kr_pairs, dim3(blocks(A.NB)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kr_finish, dim3(blocks(A.NC)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_instances = (int64_t)h.n_instances;
    if (h.g.decline != CMP_NO_DECLINE) { R.stop_head(); return 0; }
    if (A.fdr && h.n_pairs > 0) {
        FdrBuf Q;
        if (int rc = fdr_alloc(pool, A.NC, &Q)) return rc;
        unsigned flags = 0;
        if (int rc = fdr_column(st, Q, A.L, A.bound, 1, A.NC, nullptr, A.nlq3, 1, &flags)) return rc;
        if (flags & BH_RANGE) { R.stop(MC_CMP_DECLINE_FAR_TAIL); return 0; }
        if (flags & BH_TIE) { R.stop(MC_CMP_DECLINE_TIE); return 0; }
    }
    if (A.want_bed) hipLaunchKernelGGL(kr_links, dim3(blocks(A.NC)), dim3(256), 0, st, A);
    if (int rc = ph_launch_size<0>(st, A, d_head, A.NC)) return rc;
    if (int rc = ph_launch_size<1>(st, A, d_head, NR)) return rc;
    if (int rc = ph_launch_size<2>(st, A, d_head, NS)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.g.decline != CMP_NO_DECLINE) { R.stop_head(); return 0; }
    size_t nb[3];
    for (int k = 0; k < 3; ++k) nb[k] = (size_t)h.bytes[k];
    if (!cmp_fits(nb[0] + nb[1] + nb[2] + ((size_t)1 << 20))) { R.stop(MC_CMP_DECLINE_MEMORY); return 0; }
    for (int k = 0; k < 3; ++k)
        if (pool.get(&A.outp[k], nb[k] + 1)) return -10;
    hipLaunchKernelGGL(kr_write<0>, dim3(blocks(A.NC)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kr_write<1>, dim3(blocks(NR)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kr_write<2>, dim3(blocks(NS)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = fetch_out(c, c->phase.out, A.outp[0], nb[0], &res->out, &res->n_out)) return rc;
    if (int rc = fetch_out(c, c->phase.reads, A.outp[1], nb[1], &res->reads, &res->n_reads_bytes)) return rc;
    if (int rc = fetch_out(c, c->phase.bed, A.outp[2], nb[2], &res->bed, &res->n_bed)) return rc;
    S.ms_d2h = ms_since(t_d2h);
    S.n_out_bytes = (int64_t)nb[0]; S.n_reads_bytes = (int64_t)nb[1]; S.n_bed_bytes = (int64_t)nb[2];
    S.n_pairs = (int64_t)h.n_pairs; S.n_reads = (int64_t)h.n_reads; S.n_linked = (int64_t)h.n_linked;
    res->n_pairs = S.n_pairs; res->n_reads = S.n_reads; res->n_linked = S.n_linked;
    return 0;
}

int ph_call(mc_ctx *c, const mc_text_source &src, const mc_phase_options &opt, mc_phase_result *res, int32_t *status) {
    mc_phase_stats &S = c->phase.stats;
    return pipeline_call(c, S, status, "read phasing", (size_t)32 << 20, [&] { *res = mc_phase_result(); }, [&](Call &K) -> int {
        S.n_bytes = src.n_bytes; S.n_columns = opt.n_columns;
        if (!cmp_fits((size_t)src.n_bytes + 4096)) return ph_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
        char *d_text = nullptr;
        if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;
        K.feed.times(S, K.t0);
        const auto t_kernels = std::chrono::steady_clock::now();
        const int rc = ph_run(c, K.pool, d_text, src.n_bytes, opt, res, status);
        S.ms_kernels = ms_since(t_kernels) - S.ms_d2h;        // a declined call too: what ran until it declined
        return rc;
    });
}
