// mc_bedcompare.hip -- two `make_bed --vo` BED files compared per site on the GPU: one row of two-sample statistics per key
// (chrom, start, end, strand) of bed1 that bed2 also has, in bed1's order -- what compare_genomes.compare_by_position builds with
// four SciPy calls per site in a Python loop (C ABI: mc_bed_compare, mc_bed_compare_last_stats,
// mc_bed_compare_release, mc_twosample_device; Python: Device.bed_compare, compare_genomes.compare_by_position_device).  The unit
// stands in csrc/compare/, beside csrc/bed/, csrc/train/, csrc/merge/ and csrc/fastq/: no pass runs its kernels.
// Two genomes with their own assemblies are compared through a Mauve alignment: mc_xmfamap.inc, included below, builds the coordinate
// map from the XMFA text (kx_*) and lifts bed1's lines onto bed2's keys (kc_lift, in kc_probe's place; mc_bed_compare's contig tables); its
// header comment lists its declines (MC_CMP_DECLINE_XMFA_*, MC_CMP_DECLINE_LIFT_START) and its kernels' resources.
// The lines of .diffs files grouped by site are mc_sitegroup.inc (kn_parse .. kn_place, SgRun); the two pipelines included behind it
// start from it: a native sample against a control, site by site and without a model (compare_currents), is mc_curcompare.inc (the
// other kn_*); the rows of one sample's sites split in two by their currents (cluster_sites) are mc_sitecluster.inc (kl_*); the linkage of
// one sample's sites along its reads (phase_reads) is mc_readphase.inc, included last (kr_*).
// Fisher's exact test on the sites' counts and the Benjamini-Hochberg q-values of every -log10 p column (compare_genomes --fisher
// --fdr; mc_bed_compare_with's options) are mc_cmpfdr.inc, included behind it: its kernels run between kc_finish and kc_size and hand
// kc_size / kc_write the columns behind nlp_ks.  Their declines:
//   site-level   MC_CMP_DECLINE_FRAC           a SHARED line whose frac (field 5) mc_decimal.h declines or that is no count over the
//                                              line's reads (the host words the error, or float() takes what the device does not)
//                MC_CMP_DECLINE_FISHER_SELECT  a table with a mass within its derived error of the selection factor 1 + 10^-7
//                MC_CMP_DECLINE_FAR_TAIL, _TIE, _PRINT   Fisher's log10 p below -250, its printed value within its bound of a rounding
//                                              tie, a value mc_rowtext.h does not print
//   file-level   MC_CMP_DECLINE_TIE            a q-value within its column's bound of a rounding tie (no line is named)
//                MC_CMP_DECLINE_MEMORY         the columns and the sort buffers beside the rest
//
// The result is the host statement's bytes or a decline (status 1, mc_last_error; the stats say which file and line):
//   file-level   MC_CMP_DECLINE_HIGH_BYTE   a byte >= 0x80 (the host decodes the file; the device compares bytes)
//                MC_CMP_DECLINE_CONTROL     a control byte other than tab and newline ('\r' and 0x7f too: universal newlines, strip())
//                MC_CMP_DECLINE_FIELDS      a line that does not have exactly 8 tab-separated fields: the host's ValueError
//                MC_CMP_DECLINE_EMPTY       an empty chrom, start, end or strand, or an empty list (the host's float('') error)
//                MC_CMP_DECLINE_LONG_LINE   a line over 65535 bytes (spans are kept in 16 bits)
//                MC_CMP_DECLINE_ROWS        2^31 - 2 lines or more in the two files together
//                MC_CMP_DECLINE_MEMORY      the texts do not fit into free device memory beside their tables (tests:
//                                           MCALLER_CMP_DEVICE_BYTES stands for the free memory)
//                MC_CMP_DECLINE_TABLE       a key table that is full (MCALLER_CMP_TABLE_SLOTS forces one)
//   site-level   MC_CMP_DECLINE_DUPLICATE   a key that occurs twice in one file: the later line is named (the host's dict rule)
//                MC_CMP_DECLINE_NUMBER      a probability, on any line of either file, that mc_decimal.h declines (what float()
//                                           rejects, and blanks, nan, inf, long forms)
//                MC_CMP_DECLINE_DEPTH       more than TW_MAX_N = 8192 pooled values
//                MC_CMP_DECLINE_NAN         fewer than 3 pooled values or a zero pooled variance: SciPy's nan
//                MC_CMP_DECLINE_ALL_EQUAL   all pooled values equal: SciPy's nan
//                MC_CMP_DECLINE_FAR_TAIL    a log10 p below -290
//                MC_CMP_DECLINE_PRINT       a value mc_rowtext.h does not print
//                MC_CMP_DECLINE_TIE         a value within its error bound of a rounding tie (mc_twosample.h)
// Of several offending lines the first is named, bed1's before bed2's; of several reasons on it the smallest: line_flag
// (mc_textdev.h) over the lines of both texts.
//
// The two texts stand behind one another in one device buffer (a '\n' between them when bed1's last line has none), so one set of
// line starts serves both; a line is bed1's when it starts before bed2's text.  The steps (L lines, S shared sites, V values):
//   kp_count / kp_scan / kp_starts   line starts (mc_lines.h, launched by mc_textfeed.h)
//   kc_parse     a lane per line: ByteClass, the seven tabs (tabs_pack), the key's KeyHash, the list's comma count, EVERY number's
//                grammar (mc_decimal.h: the host calls float() on every line, shared or not); bed1's line count
//   kc_insert    twice: bed2's keys, then bed1's, each into a key table of its own (kt_claim; ids are lines).  An equal key is a
//                duplicate: the slot keeps the smaller line by atomicMin and the larger one is named, whatever order the lanes
//                arrive in
//   kc_probe     a lane per bed1 line against bed2's table (kt_find) -> the matching line or none, a 0 / 1 flag; the longest
//                probe in slots read, the empty one included
//   kp_scan      the flags: bed1's matched lines numbered in file order (no atomicAdd decides an order anywhere)
//   kc_sites     a lane per bed1 line: its site's two lines and value counts; kp_scan x 2: the samples' offsets
//   kc_tokens    a lane per site and sample: the spans of its numbers
//   kc_values    a lane per NUMBER: mc_decimal.h -> one array per sample
//   kc_rank_small  a WAVE per site of up to 64 pooled values: a value a lane, the others broadcast one after the other
//   kc_rank_large  a WORKGROUP per site of up to 8192 (two instances: up to 512 and beyond): the values in LDS, a thread takes four
//                of its values per sweep over them.
//                Both make, for every pooled value, the four counts of mc_twosample.h -> twice the rank sum and the tie term in 64-bit
//                integers, D by fp64 max (exact, order-free), the means in NumPy's own order of additions (mc_npsum.h), the sums of
//                squares compensated in an order fixed by the row order.
//                No sort, no floating-point atomic
//   kc_finish    a lane per site: tw_finish -> the nine values, their bounds, the status bits
//   kc_size / kp_scan / kc_write   a lane per site: the row's length, its place, its bytes (digits: mc_rowtext.h; keys, frac and
//                depth copied from the texts)
// Resources (tools/kres.py, gfx950; no kernel of the unit spills or uses scratch):
//   kc_rank_small  256 threads = four sites a workgroup, 60 VGPRs, no LDS, 8 waves a SIMD: a site's values never leave registers
//   kc_rank_large  two instances, 146 VGPRs each (3 waves a SIMD by registers):
//                  <512, 64, 128>     sites of 65 .. 512 pooled values, 128 threads, 4176 bytes of LDS: registers set the occupancy (3).
//                                     At depths 15 .. 60 a file's sites are of 65 .. 120: they neither hold 64 KB of LDS nor leave
//                                     most of 256 threads idle
//                  <8192, 512, 256>   sites up to the cap, 256 threads, 65696 bytes of LDS (8192 doubles and the reductions' few
//                                     words): LDS sets the occupancy, two workgroups a CU of its 160 KB (2 waves a SIMD)
//                  Every lane of a wave reads the same word of LDS in the sweep (a broadcast, no bank conflict); the sweep is
//                  compare-bound (four compares per pair of values), so a site of 8192 costs 2^26 compares on one CU: the cap
//                  is where that stays in the milliseconds.  The two means are summed by one thread each (NumPy's order is serial
//                  within a leaf of 128): 8191 additions at the most, beside 2^26 compares
//   kc_finish      82 VGPRs, 5 waves a SIMD (the continued fraction of mc_tstat.h, four tails at three points each)
//   kc_parse       42 VGPRs: mc_decimal.h on every number of the line, a lane per line -- the unit's longest kernel since (0.64 of
//                  1.45 ms at 10^4 sites, profiles/compare_kernel_stats.csv); a shared site's numbers are read again by kc_values
#include "../mc_textfeed.h"
#include "../mc_decimal.h"
#include "../mc_twosample.h"
#include "../mc_fisher.h"
#include "../mc_bh.h"

#include <cstdio>
#include <cstring>

namespace {

constexpr unsigned long long CMP_NO_DECLINE = ~0ull;
constexpr int CR_THREADS = 256;
constexpr int CR_MID = 512, CR_MID_THREADS = 128;      // kc_rank_large's smaller instance: sites of 65 .. 512 pooled values

struct CmpHead {                             // device-side result block (copied to the host as it is)
    KpHead kp;
    unsigned long long decline;              // min over the offending lines of line << 8 | reason (~0: none)
    long long n_lines1;                      // lines that start before bed2's text
    long long n_sites, n_x, n_y, out_bytes;  // totals of the scans
    unsigned long long n_small, n_large;     // sites each rank kernel took
    int longest_probe, deepest;
    unsigned long long n_unaligned;          // (a lifted comparison) bed1's lines that have no image
};

// a lifted comparison (mc_xmfamap.inc): the resident map, genome 1's contig names in a key table, both genomes' offsets
struct LiftDev {
    const unsigned long long *map;
    int64_t n1, nc1, nc2;
    const unsigned long long *ctable;
    uint64_t cmask;
    const char *ids1, *ids2;
    const long long *id_off1, *id_off2, *off1, *off2;
};

struct CmpArgs {
    const char *text;
    int64_t n_bytes, off2, n_nl, n_lines, n_lines1;
    const long long *line_start;
    CmpHead *head;
    // per line
    uint4 *span;                             // t0 | t1 << 16, t2 | t3 << 16, t4 | t5 << 16, t6 | length << 16 (0: not a line the tables take)
    uint64_t *hash;
    uint32_t *n_vals;
    long long *match, *flag, *site_of;       // bed1 lines: the matching line or -1, 0 / 1, the scan
    uint64_t hash_mask;
    unsigned long long *table[2];            // bed1's keys, bed2's keys
    uint64_t mask[2];
    // per site
    int64_t S;
    long long *line1, *line2, *cnt1, *cnt2, *off1, *off2v, *row_len, *row_off;
    // per value
    int64_t n_x, n_y;
    long long *tok_b;
    uint32_t *tok_n, *tok_line;
    double *vals;                            // x[0, n_x) then y[0, n_y)
    TwSite *sites;
    double *out9, *bound9;
    int32_t *status;
    char *out;
    int lifted;                              // 1: kc_lift matched the lines; a row carries the image's key behind bed1's
    LiftDev lift;
    // mc_bed_compare_with (mc_cmpfdr.inc): the columns behind nlp_ks
    int fisher, fdr, n_extra;                // n_extra: fisher + (4 + fisher) fdr columns a row
    double *logs, *log_bound;                // per site: the log10 p of the four tests and of Fisher's before rounding, their bounds
    double *extra;                           // per site: the n_extra printed values
};

constexpr int CMP_LOGS = 5;

__device__ __forceinline__ TabSpan cmp_line(const CmpArgs &A, int64_t li) { return tabs_unpack(A.span[li]); }

__global__ __launch_bounds__(256) void kc_parse(CmpArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_lines = A.head->kp.n_lines;
    if (li >= n_lines) return;
    const int64_t b = A.line_start[li];
    const int64_t e = li < A.n_nl ? (int64_t)A.line_start[li + 1] - 1 : A.n_bytes;
    A.span[li] = make_uint4(0u, 0u, 0u, 0u);
    A.hash[li] = 0;
    A.n_vals[li] = 0;
    if (b < A.off2 && (li + 1 >= n_lines || (int64_t)A.line_start[li + 1] >= A.off2)) A.head->n_lines1 = li + 1;      // bed1's last line alone
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_LONG_LINE); return; }
    const char *t = A.text + b;
    const int len = (int)(e - b);
    ByteClass bad;
    int tab[7] = {0, 0, 0, 0, 0, 0, 0}, nt = 0, commas = 0;
    for (int i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)t[i];
        bad.see(c);
        if (c == '\t') {
#pragma unroll
            for (int k = 0; k < 7; ++k) tab[k] = nt == k ? i : tab[k];
            ++nt;
        }
        commas += (c == ',' && nt == 7) ? 1 : 0;
    }
    if (bad.hi) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CONTROL); return; }
    if (nt != 7) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_FIELDS); return; }
    // chrom [0, t0), start (t0, t1), end (t1, t2), strand (t4, t5), the list (t6, len)
    if (tab[0] == 0 || tab[1] - tab[0] == 1 || tab[2] - tab[1] == 1 || tab[5] - tab[4] == 1 || len - tab[6] == 1) {
        line_flag(&A.head->decline, li, MC_CMP_DECLINE_EMPTY);
        return;
    }
    // every number of every line, shared or not: the host calls float() on all of them before it looks at a key
    bool bad_number = false;
    for (int p = tab[6] + 1, tb = tab[6] + 1; p <= len; ++p)
        if (p == len || t[p] == ',') {
            double d;
            bad_number |= !dc_parse(t + tb, p - tb, &d);
            tb = p + 1;
        }
    if (bad_number) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_NUMBER); return; }
    KeyHash H;
    H.span(t, tab[0]); H.sep();
    H.span(t + tab[0] + 1, tab[1] - tab[0] - 1); H.sep();
    H.span(t + tab[1] + 1, tab[2] - tab[1] - 1); H.sep();
    H.span(t + tab[4] + 1, tab[5] - tab[4] - 1);
    A.hash[li] = H.done(A.hash_mask);
    A.n_vals[li] = (uint32_t)commas + 1u;
    A.span[li] = tabs_pack(tab, len);
}

// the keys of lines a and b, byte for byte: chrom, start and end are one span with its tabs, the strand another
__device__ __forceinline__ bool cmp_same_key(const CmpArgs &A, int64_t a, int64_t b) {
    const TabSpan La = cmp_line(A, a), Lb = cmp_line(A, b);
    if (La.t[0] != Lb.t[0] || La.t[1] != Lb.t[1] || La.t[2] != Lb.t[2] || La.t[5] - La.t[4] != Lb.t[5] - Lb.t[4]) return false;
    const char *pa = A.text + A.line_start[a], *pb = A.text + A.line_start[b];
    return same_bytes(pa, pb, La.t[2]) && same_bytes(pa + La.t[4] + 1, pb + Lb.t[4] + 1, La.t[5] - La.t[4] - 1);
}

// which = 0: bed1's lines [0, n_lines1) into table[0]; 1: bed2's [n_lines1, n_lines) into table[1]
__global__ __launch_bounds__(256) void kc_insert(CmpArgs A, int which) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x + (which ? A.n_lines1 : 0);
    if (li >= (which ? A.n_lines : A.n_lines1) || cmp_line(A, li).len == 0) return;      // (a line kc_parse left out)
    unsigned long long *table = A.table[which];
    const uint64_t h = A.hash[li];
    const KtHit hit = kt_claim(table, A.mask[which], h, li, [&](int64_t r) { return A.hash[r] == h && cmp_same_key(A, li, r); });
    if (hit.slot < 0) line_flag(&A.head->decline, li, MC_CMP_DECLINE_TABLE);
    else if (!hit.claimed) {
        // the same key twice: the slot keeps the smaller line, the larger of the two that met here is named
        const unsigned long long old = atomicMin(&table[hit.slot], kt_word(h, li));
        const int64_t other = (int64_t)(old & 0xffffffffull) - 1;
        line_flag(&A.head->decline, other > li ? other : li, MC_CMP_DECLINE_DUPLICATE);
    }
}

__global__ __launch_bounds__(256) void kc_probe(CmpArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1) return;
    long long found = -1;
    int looked = 0;                                                    // slots read, the empty one included
    if (cmp_line(A, li).len != 0) {
        const uint64_t h = A.hash[li];                                 // (the table is complete: kc_insert ran before)
        const KtHit hit = kt_find(A.table[1], A.mask[1], h, [&](int64_t r) { return A.hash[r] == h && cmp_same_key(A, li, r); });
        found = hit.id;
        looked = (int)hit.looked;
    }
    A.match[li] = found;
    A.flag[li] = found >= 0 ? 1 : 0;
    if (looked > A.head->longest_probe) atomicMax(&A.head->longest_probe, looked);
}

__global__ __launch_bounds__(256) void kc_sites(CmpArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1 || A.match[li] < 0) return;
    const long long s = A.site_of[li], r = A.match[li];
    if (s < 0 || s >= A.S) return;                                     // (cannot be: the scan counted these lines)
    const long long c1 = A.n_vals[li], c2 = A.n_vals[r];
    A.line1[s] = li; A.line2[s] = r;
    A.cnt1[s] = c1; A.cnt2[s] = c2;
    const long long n = c1 + c2;
    if (n > TW_MAX_N) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_DEPTH); A.cnt1[s] = 0; A.cnt2[s] = 0; }
    const int deep = (int)(n > 0x7fffffffll ? 0x7fffffffll : n);
    if (deep > A.head->deepest) atomicMax(&A.head->deepest, deep);
}

// a lane per site and sample: where its numbers stand (the list was counted by its commas)
__global__ __launch_bounds__(256) void kc_tokens(CmpArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * A.S) return;
    const int64_t s = i >> 1;
    const int side = (int)(i & 1);
    const long long li = side ? A.line2[s] : A.line1[s];
    const long long at = side ? A.n_x + A.off2v[s] : A.off1[s], k = side ? A.cnt2[s] : A.cnt1[s];
    const TabSpan L = cmp_line(A, li);
    const int64_t b = A.line_start[li];
    long long j = 0;
    int tb = L.t[6] + 1;
    for (int p = L.t[6] + 1; p <= L.len && j < k; ++p)
        if (p == L.len || A.text[b + p] == ',') {
            A.tok_b[at + j] = b + tb; A.tok_n[at + j] = (uint32_t)(p - tb); A.tok_line[at + j] = (uint32_t)li;
            ++j; tb = p + 1;
        }
}

__global__ __launch_bounds__(256) void kc_values(CmpArgs A) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= A.n_x + A.n_y) return;
    double d = 0.0;
    if (!dc_parse(A.text + A.tok_b[v], (int)A.tok_n[v], &d)) line_flag(&A.head->decline, A.tok_line[v], MC_CMP_DECLINE_NUMBER);
    A.vals[v] = d;
}

// ---- the ranks ----
struct RankArgs {
    const double *x, *y;
    const long long *x_off, *x_cnt, *y_off, *y_cnt;
    int64_t S;
    TwSite *sites;
    unsigned long long *n_small, *n_large;
};

__device__ __forceinline__ TsSum ts_shfl_down(const TsSum &a, int o) {
    TsSum r;
    r.s = __shfl_down(a.s, o); r.c = __shfl_down(a.c, o);
    return r;
}

__global__ __launch_bounds__(CR_THREADS) void kc_rank_small(RankArgs R) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * (CR_THREADS / 64) + (threadIdx.x >> 6);     // (the same for the whole wave)
    if (s >= R.S) return;
    const long long n1 = R.x_cnt[s], n2 = R.y_cnt[s], n = n1 + n2;
    if (n > 64) return;
    TwSite out;
    out.n1 = n1; out.n2 = n2;
    if (n1 < 1 || n2 < 1) { if (lane == 0) R.sites[s] = out; return; }
    const bool mine = lane < n, of_x = lane < n1;
    const double v = mine ? (of_x ? R.x[R.x_off[s] + lane] : R.y[R.y_off[s] + lane - n1]) : 0.0;
    long long x_lt = 0, x_le = 0, y_lt = 0, y_le = 0;
    for (int j = 0; j < (int)n; ++j) {
        const double w = __shfl(v, j);
        if (j < n1) { x_lt += w < v; x_le += w <= v; }
        else { y_lt += w < v; y_le += w <= v; }
    }
    // the means in NumPy's order (one leaf of mc_npsum.h: n <= 64); every lane adds the same words: the same bits in all
    const NsPlain px{R.x + R.x_off[s]}, py{R.y + R.y_off[s]};
    const double m1 = tw_np_sum(px, n1) / (double)n1, m2 = tw_np_sum(py, n2) / (double)n2;
    TsSum q1, q2;
    for (int j = 0; j < (int)n; ++j) {
        const double w = __shfl(v, j);
        if (j < n1) { const double d = w - m1; q1.add(d * d); }
        else { const double d = w - m2; q2.add(d * d); }
    }
    TwCount C;
    if (mine) C.value(of_x, x_lt, x_le, y_lt, y_le, n1, n2);
    for (int o = 32; o > 0; o >>= 1) {
        C.r1x2 += __shfl_xor(C.r1x2, o);
        C.tie += __shfl_xor(C.tie, o);
        const double d = __shfl_xor(C.D, o);
        C.D = d > C.D ? d : C.D;
    }
    if (lane == 0) {
        out.r1x2 = C.r1x2; out.tie = C.tie; out.D = C.D;
        out.mean1 = m1; out.mean2 = m2; out.ss1 = q1.value(); out.ss2 = q2.value();
        R.sites[s] = out;
        atomicAdd(R.n_small, 1ull);
    }
}

// the workgroup's compensated sums, one per thread, into one: down the lanes of each wave, then the waves in turn -- a fixed order
template <int THREADS>
__device__ __forceinline__ TsSum cr_block_sum(TsSum a, double *s_s, double *s_c) {
    for (int o = 32; o > 0; o >>= 1) a.merge(ts_shfl_down(a, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_s[threadIdx.x >> 6] = a.s; s_c[threadIdx.x >> 6] = a.c; }
    __syncthreads();
    TsSum t;
    for (int w = 0; w < THREADS / 64; ++w) { TsSum o; o.s = s_s[w]; o.c = s_c[w]; t.merge(o); }
    return t;
}

// sites of LO < n <= CAP pooled values, a workgroup of THREADS each: <CR_MID, 64, 128> and <TW_MAX_N, CR_MID, 256>
template <int CAP, int LO, int THREADS>
__global__ __launch_bounds__(THREADS) void kc_rank_large(RankArgs R) {
    __shared__ double s_v[CAP];
    __shared__ double s_s[THREADS / 64], s_c[THREADS / 64], s_d[THREADS / 64];
    __shared__ long long s_r[THREADS / 64], s_t[THREADS / 64];
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x;
    const long long n1 = R.x_cnt[s], n2 = R.y_cnt[s], n = n1 + n2;
    if (n <= LO || n > CAP) return;
    TwSite out;
    out.n1 = n1; out.n2 = n2;
    if (n1 < 1 || n2 < 1) { if (tid == 0) R.sites[s] = out; return; }
    const double *x = R.x + R.x_off[s], *y = R.y + R.y_off[s];
    for (long long i = tid; i < n; i += THREADS) s_v[i] = i < n1 ? x[i] : y[i - n1];
    __syncthreads();
    // the means in NumPy's order of additions (mc_npsum.h): one thread a sample, the first lane of two waves, out of LDS
    if (tid == 0) { const NsPlain px{s_v}; s_s[0] = tw_np_sum(px, n1); }
    if (tid == 64) { const NsPlain py{s_v + n1}; s_s[1] = tw_np_sum(py, n2); }
    __syncthreads();
    const double m1 = s_s[0] / (double)n1, m2 = s_s[1] / (double)n2;
    // the sums of squares about them: thread k takes the values k, k + 256, ... of each sample
    TsSum q1, q2;
    for (long long i = tid; i < n1; i += THREADS) { const double d = s_v[i] - m1; q1.add(d * d); }
    for (long long i = tid; i < n2; i += THREADS) { const double d = s_v[n1 + i] - m2; q2.add(d * d); }
    const double ss1 = cr_block_sum<THREADS>(q1, s_s, s_c).value(), ss2 = cr_block_sum<THREADS>(q2, s_s, s_c).value();
    // the counts: four of the thread's values per sweep over all of them (every lane reads the same word of LDS: a broadcast)
    TwCount C;
    for (long long base = tid; base < n; base += 4 * THREADS) {
        double v[4];
        long long x_lt[4] = {0, 0, 0, 0}, x_le[4] = {0, 0, 0, 0}, y_lt[4] = {0, 0, 0, 0}, y_le[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) { const long long i = base + (long long)k * THREADS; v[k] = i < n ? s_v[i] : 0.0; }
        for (long long j = 0; j < n1; ++j) {
            const double w = s_v[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) { x_lt[k] += w < v[k]; x_le[k] += w <= v[k]; }
        }
        for (long long j = n1; j < n; ++j) {
            const double w = s_v[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) { y_lt[k] += w < v[k]; y_le[k] += w <= v[k]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = base + (long long)k * THREADS;
            if (i < n) C.value(i < n1, x_lt[k], x_le[k], y_lt[k], y_le[k], n1, n2);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        C.r1x2 += __shfl_xor(C.r1x2, o);
        C.tie += __shfl_xor(C.tie, o);
        const double d = __shfl_xor(C.D, o);
        C.D = d > C.D ? d : C.D;
    }
    __syncthreads();
    if ((tid & 63) == 0) { s_r[tid >> 6] = C.r1x2; s_t[tid >> 6] = C.tie; s_d[tid >> 6] = C.D; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < THREADS / 64; ++w) {
            out.r1x2 += s_r[w]; out.tie += s_t[w];
            out.D = s_d[w] > out.D ? s_d[w] : out.D;
        }
        out.mean1 = m1; out.mean2 = m2; out.ss1 = ss1; out.ss2 = ss2;
        R.sites[s] = out;
        atomicAdd(R.n_large, 1ull);
    }
}

// x_cnt / y_cnt of a site no rank kernel takes: its TwSite with the counts alone (tw_finish names it)
__global__ __launch_bounds__(256) void kc_finish(const TwSite *__restrict__ sites, const long long *__restrict__ x_cnt,
                                                 const long long *__restrict__ y_cnt, int64_t S, double *__restrict__ out9,
                                                 double *__restrict__ bound9, int32_t *__restrict__ status, double *__restrict__ logs,
                                                 double *__restrict__ log_bound) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    double o[TW_N_OUT], b[TW_N_OUT], l[4];
    int st;
    if (x_cnt[s] + y_cnt[s] > TW_MAX_N) {
        st = TW_DEEP;
        for (int i = 0; i < TW_N_OUT; ++i) { o[i] = __builtin_nan(""); b[i] = 0.0; }
        for (int i = 0; i < 4; ++i) l[i] = __builtin_nan("");
    } else {
        st = tw_finish(sites[s], o, b, l);
    }
    for (int i = 0; i < TW_N_OUT; ++i) { out9[s * TW_N_OUT + i] = o[i]; bound9[s * TW_N_OUT + i] = b[i]; }
    status[s] = st;
    if (logs)                                                          // (mc_bed_compare_with's fdr: the q-values start from these)
        for (int i = 0; i < 4; ++i) { logs[s * CMP_LOGS + i] = l[i]; log_bound[s * CMP_LOGS + i] = b[5 + i]; }
}

// the row of site s into the sink: the key, frac and depth of the two lines as they stand, the nine numbers
template <class Sink>
__device__ __forceinline__ void cmp_put_row(const CmpArgs &A, int64_t s, Sink &o) {
    const long long l1 = A.line1[s], l2 = A.line2[s];
    const TabSpan L1 = cmp_line(A, l1), L2 = cmp_line(A, l2);
    const char *p1 = A.text + A.line_start[l1], *p2 = A.text + A.line_start[l2];
    for (int i = 0; i <= L1.t[2]; ++i) o.put(p1[i]);                   // chrom, start, end and the tab behind each
    for (int i = L1.t[4] + 1; i <= L1.t[5]; ++i) o.put(p1[i]);         // strand, its tab
    if (A.lifted) {                                                    // the image: bed2's key as it stands
        for (int i = 0; i <= L2.t[2]; ++i) o.put(p2[i]);
        for (int i = L2.t[4] + 1; i <= L2.t[5]; ++i) o.put(p2[i]);
    }
    for (int i = L1.t[3] + 1; i <= L1.t[4]; ++i) o.put(p1[i]);         // frac1
    for (int i = L1.t[5] + 1; i <= L1.t[6]; ++i) o.put(p1[i]);         // depth1
    for (int i = L2.t[3] + 1; i <= L2.t[4]; ++i) o.put(p2[i]);
    for (int i = L2.t[5] + 1; i <= L2.t[6]; ++i) o.put(p2[i]);
    for (int i = 0; i < TW_N_OUT; ++i) {
        rt_put_num(o, rt_num_of(A.out9[s * TW_N_OUT + i]));
        o.put(i + 1 < TW_N_OUT || A.n_extra ? '\t' : '\n');
    }
    for (int i = 0; i < A.n_extra; ++i) {                              // nlp_fisher, the q-values
        rt_put_num(o, rt_num_of(A.extra[s * A.n_extra + i]));
        o.put(i + 1 < A.n_extra ? '\t' : '\n');
    }
}

__global__ __launch_bounds__(256) void kc_size(CmpArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    const int st = A.status[s];
    A.row_len[s] = 0;
    if (st) {
        const int reason = (st & TW_ALL_EQUAL) ? MC_CMP_DECLINE_ALL_EQUAL : (st & (TW_BAD_N | TW_ZERO_VAR)) ? MC_CMP_DECLINE_NAN
                         : (st & TW_DEEP) ? MC_CMP_DECLINE_DEPTH : (st & TW_FAR_TAIL) ? MC_CMP_DECLINE_FAR_TAIL
                         : (st & TW_UNPRINTABLE) ? MC_CMP_DECLINE_PRINT : MC_CMP_DECLINE_TIE;
        line_flag(&A.head->decline, A.line1[s], reason);
        return;
    }
    for (int i = 0; i < A.n_extra; ++i) {                              // (a NaN: the site's line has declined the file with its own reason)
        const double v = A.extra[s * A.n_extra + i];
        if (v != v) return;
        if (!rt_num_of(v).ok) { line_flag(&A.head->decline, A.line1[s], MC_CMP_DECLINE_PRINT); return; }
    }
    RtCount count;
    cmp_put_row(A, s, count);
    A.row_len[s] = count.n;
}

__global__ __launch_bounds__(256) void kc_write(CmpArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    const long long at = A.row_off[s], len = A.row_len[s];
    if (at < 0 || at + len > A.head->out_bytes) return;                // (cannot be: the scan counted these bytes)
    RtStore store{A.out + at};
    cmp_put_row(A, s, store);
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

const char *cmp_reason_text(int reason) {
    switch (reason) {
        case MC_CMP_DECLINE_HIGH_BYTE: return "a byte >= 0x80";
        case MC_CMP_DECLINE_CONTROL: return "a control byte other than tab and newline";
        case MC_CMP_DECLINE_FIELDS: return "a line that does not have 8 tab-separated fields";
        case MC_CMP_DECLINE_EMPTY: return "an empty key field or an empty probability list";
        case MC_CMP_DECLINE_LONG_LINE: return "a line longer than 65535 bytes";
        case MC_CMP_DECLINE_ROWS: return "2^31 - 2 lines or more";
        case MC_CMP_DECLINE_MEMORY: return "the texts do not fit into free device memory beside their tables";
        case MC_CMP_DECLINE_TABLE: return "the key table is full";
        case MC_CMP_DECLINE_DUPLICATE: return "a key that occurs twice in one file";
        case MC_CMP_DECLINE_NUMBER: return "a probability the device's decimal reader declines";
        case MC_CMP_DECLINE_DEPTH: return "a site with more than 8192 pooled values";
        case MC_CMP_DECLINE_NAN: return "a site with fewer than 3 pooled values or a zero pooled variance";
        case MC_CMP_DECLINE_ALL_EQUAL: return "a site whose pooled values are all equal";
        case MC_CMP_DECLINE_FAR_TAIL: return "a log10 p below -290 (Fisher's test: -250)";
        case MC_CMP_DECLINE_PRINT: return "a value the device's row writer does not print";
        case MC_CMP_DECLINE_TIE: return "a value within its error bound of a rounding tie";
        case MC_CMP_DECLINE_LIFT_START: return "a start that is not plain digits";
        case MC_CMP_DECLINE_FRAC: return "a shared line whose frac is not a count over its reads";
        case MC_CMP_DECLINE_FISHER_SELECT: return "a table of Fisher's test with a mass within its error of the selection factor";
    }
    return "unknown";
}

// file: 1, 2 or 0; line: in that file, -1: none
int cmp_decline(mc_ctx *c, int32_t *status, int reason, int file, long long line) {
    static const char *const nouns[2] = {"bed1", "bed2"};
    return decline_in_file(c->cmp.stats, status, "comparison", cmp_reason_text(reason), nouns, reason, file, line);
}

int cmp_decline_head(mc_ctx *c, int32_t *status, const CmpHead &h) {
    const long long line = decline_line(h.decline);
    const bool first = line < h.n_lines1;
    return cmp_decline(c, status, decline_reason(h.decline), first ? 1 : 2, first ? line : line - h.n_lines1);
}

// device_fits, or (tests) as if MCALLER_CMP_DEVICE_BYTES were all the device had free
bool cmp_fits(size_t bytes) { return fits("MCALLER_CMP_DEVICE_BYTES", bytes); }

// (tests: long probe chains) the mask every key hash of the unit is cut to: MCALLER_CMP_HASH_MASK, hexadecimal
uint64_t cmp_hash_mask() {
    const char *hm = getenv("MCALLER_CMP_HASH_MASK");
    return hm && *hm ? strtoull(hm, nullptr, 16) : ~0ull;
}

int launch_ranks(hipStream_t st, const RankArgs &R) {
    if (R.S <= 0) return 0;
    hipLaunchKernelGGL(kc_rank_small, dim3((unsigned)((R.S + 3) / 4)), dim3(CR_THREADS), 0, st, R);
    hipLaunchKernelGGL((kc_rank_large<CR_MID, 64, CR_MID_THREADS>), dim3((unsigned)R.S), dim3(CR_MID_THREADS), 0, st, R);
    hipLaunchKernelGGL((kc_rank_large<TW_MAX_N, CR_MID, CR_THREADS>), dim3((unsigned)R.S), dim3(CR_THREADS), 0, st, R);
    HIP_TRY(hipGetLastError());
    return 0;
}

#include "mc_xmfamap.inc"
#include "mc_cmpfdr.inc"
#include "mc_sitegroup.inc"
#include "mc_curcompare.inc"
#include "mc_sitecluster.inc"
#include "mc_readphase.inc"

// The texts are on the device (d_text[0, n): bed1's, a newline if it lacked its last, bed2's from off2 on; padded): everything behind that
// (lift: the device side of a lifted comparison, nullptr: keys are matched as they stand)
int cmp_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, int64_t off2, const char **out, int64_t *n_out, int64_t *n_sites,
            int32_t *status, const LiftDev *lift, const mc_cmp_options *opt) {
    mc_cmp_stats &S = c->cmp.stats;
    hipStream_t st = c->stream;
    if (n == 0) return 0;
    CmpHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline = CMP_NO_DECLINE;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, d_text, n, &d_head->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t n_nl = h.kp.n_newlines;
    if (too_many_lines(n_nl)) return cmp_decline(c, status, MC_CMP_DECLINE_ROWS, 0, -1);
    const size_t cap = (size_t)n_nl + 2;
    if (!cmp_fits(cap * (8 + 16 + 8 + 4 + 24 + 64) + ((size_t)1 << 20))) return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    if (int rc = lines_starts(pool, st, d_text, n, n_nl, tile_off, &d_head->kp, &line_start)) return rc;
    CmpArgs A = {};
    A.text = d_text; A.n_bytes = n; A.off2 = off2; A.n_nl = n_nl; A.line_start = line_start; A.head = d_head;
    if (lift) { A.lifted = 1; A.lift = *lift; }
    A.hash_mask = cmp_hash_mask();
    if (pool.get(&A.span, cap) || pool.get(&A.hash, cap) || pool.get(&A.n_vals, cap) || pool.get(&A.match, cap) || pool.get(&A.flag, cap) ||
        pool.get(&A.site_of, cap))
        return -10;
    hipLaunchKernelGGL(kc_parse, dim3(blocks((int64_t)cap)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t L = h.kp.n_lines, L1 = h.n_lines1, L2 = L - L1;
    S.n_lines1 = L1; S.n_lines2 = L2;
    if (h.decline != CMP_NO_DECLINE) return cmp_decline_head(c, status, h);
    A.n_lines = L; A.n_lines1 = L1;
    S.n_keys2 = L2;
    if (L1 > 0 && (L2 > 0 || lift)) {                                  // (a lifted comparison counts bed1's lines without an image in any case)
        A.mask[0] = table_slots(L1, 64, "MCALLER_CMP_TABLE_SLOTS") - 1; A.mask[1] = table_slots(L2, 64, "MCALLER_CMP_TABLE_SLOTS") - 1;
        S.table_slots = (int64_t)A.mask[1] + 1;
        if (!cmp_fits((A.mask[0] + A.mask[1] + 2) * 8 + ((size_t)1 << 20))) return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
        for (int w = 0; w < 2; ++w)
            if (int rc = table_get(pool, st, &A.table[w], A.mask[w] + 1)) return rc;
        if (L2 > 0) hipLaunchKernelGGL(kc_insert, dim3(blocks(L2)), dim3(256), 0, st, A, 1);
        hipLaunchKernelGGL(kc_insert, dim3(blocks(L1)), dim3(256), 0, st, A, 0);
        if (lift) hipLaunchKernelGGL(kc_lift, dim3(blocks(L1)), dim3(256), 0, st, A);
        else hipLaunchKernelGGL(kc_probe, dim3(blocks(L1)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.flag, L1, A.site_of, &d_head->n_sites);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.decline != CMP_NO_DECLINE) return cmp_decline_head(c, status, h);
        S.longest_probe = h.longest_probe;
        c->cmp.unaligned = (int64_t)h.n_unaligned;
    }
    const int64_t NS = h.n_sites;
    S.n_sites = NS;
    if (NS > 0) {
        A.S = NS;
        const size_t ns = (size_t)NS;
        if (!cmp_fits(ns * (8 * 8 + sizeof(TwSite) + 2 * 8 * TW_N_OUT + 4) + ((size_t)1 << 20)))
            return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
        if (pool.get(&A.line1, ns) || pool.get(&A.line2, ns) || pool.get(&A.cnt1, ns) || pool.get(&A.cnt2, ns) || pool.get(&A.off1, ns) ||
            pool.get(&A.off2v, ns) || pool.get(&A.row_len, ns) || pool.get(&A.row_off, ns) || pool.get(&A.sites, ns) ||
            pool.get(&A.out9, ns * TW_N_OUT) || pool.get(&A.bound9, ns * TW_N_OUT) || pool.get(&A.status, ns))
            return -10;
        if (opt && (opt->fisher || opt->fdr)) {                        // the columns behind nlp_ks, and the sort buffers of their q-values
            A.fisher = opt->fisher != 0; A.fdr = opt->fdr != 0;
            A.n_extra = A.fisher + (4 + A.fisher) * A.fdr;
            if (!cmp_fits(ns * (8 * 8 + sizeof(TwSite) + 2 * 8 * TW_N_OUT + 4) + ns * 8 * (2 * CMP_LOGS + (size_t)A.n_extra) + (A.fdr ? fdr_bytes(NS) : 0) +
                          ((size_t)1 << 20)))
                return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
            if (pool.get(&A.logs, ns * CMP_LOGS) || pool.get(&A.log_bound, ns * CMP_LOGS) || pool.get(&A.extra, ns * (size_t)A.n_extra)) return -10;
        }
        hipLaunchKernelGGL(kc_sites, dim3(blocks(L1)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt1, NS, A.off1, &d_head->n_x);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt2, NS, A.off2v, &d_head->n_y);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;
        S.deepest_site = h.deepest;
        if (h.decline != CMP_NO_DECLINE) return cmp_decline_head(c, status, h);
        A.n_x = h.n_x; A.n_y = h.n_y;
        S.n_values = h.n_x + h.n_y;
        const size_t nv = (size_t)(h.n_x + h.n_y);
        if (!cmp_fits(nv * 24 + ((size_t)1 << 20))) return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
        if (pool.get(&A.tok_b, nv) || pool.get(&A.tok_n, nv) || pool.get(&A.tok_line, nv) || pool.get(&A.vals, nv)) return -10;
        hipLaunchKernelGGL(kc_tokens, dim3(blocks(2 * NS)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kc_values, dim3(blocks((int64_t)nv)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;           // (a declined number: no rank is taken of it)
        if (h.decline != CMP_NO_DECLINE) return cmp_decline_head(c, status, h);
        RankArgs R = {A.vals, A.vals + A.n_x, A.off1, A.cnt1, A.off2v, A.cnt2, NS, A.sites, &d_head->n_small, &d_head->n_large};
        if (int rc = launch_ranks(st, R)) return rc;
        hipLaunchKernelGGL(kc_finish, dim3(blocks(NS)), dim3(256), 0, st, (const TwSite *)A.sites, (const long long *)A.cnt1,
                           (const long long *)A.cnt2, NS, A.out9, A.bound9, A.status, A.logs, A.log_bound);
        unsigned bh_flags = 0;
        if (A.n_extra)
            if (int rc = cmp_extra_columns(c, pool, A, &bh_flags)) return rc;
        hipLaunchKernelGGL(kc_size, dim3(blocks(NS)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.row_len, NS, A.row_off, &d_head->out_bytes);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;
        S.n_rank_small = (int64_t)h.n_small; S.n_rank_large = (int64_t)h.n_large;
        if (h.decline != CMP_NO_DECLINE) return cmp_decline_head(c, status, h);
        if (bh_flags & BH_RANGE) return cmp_decline(c, status, MC_CMP_DECLINE_FAR_TAIL, 0, -1);
        if (bh_flags & BH_TIE) return cmp_decline(c, status, MC_CMP_DECLINE_TIE, 0, -1);
        const size_t ob = (size_t)h.out_bytes;
        if (!cmp_fits(ob + ((size_t)1 << 20))) return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
        if (pool.get(&A.out, ob)) return -10;
        hipLaunchKernelGGL(kc_write, dim3(blocks(NS)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        const auto t_d2h = std::chrono::steady_clock::now();
        if (int rc = fetch_out(c, c->cmp.out, A.out, ob, out, n_out)) return rc;
        S.ms_d2h = ms_since(t_d2h);
        S.n_out_bytes = (int64_t)ob;
        *n_sites = NS;
        return 0;
    }
    return 0;
}

// a contig table's arrays onto the device (the pool's) -> the device pointers
int lift_upload(Pool &pool, hipStream_t st, const mc_contig_table *t, const char **ids, const long long **id_off, const long long **off) {
    const size_t nc = (size_t)t->n_contigs, n_ids = (size_t)t->id_off[nc];
    char *d_ids = nullptr;
    long long *d_id_off = nullptr, *d_off = nullptr;
    if (pool.get(&d_ids, n_ids + 1) || pool.get(&d_id_off, nc + 1) || pool.get(&d_off, nc + 1)) return -10;
    if (n_ids) HIP_TRY(hipMemcpyAsync(d_ids, t->ids, n_ids, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_id_off, t->id_off, (nc + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, t->off, (nc + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                                 // (the host arrays are the caller's)
    *ids = d_ids; *id_off = d_id_off; *off = d_off;
    return 0;
}

// the device side of a lifted comparison: the contig tables, genome 1's names in a key table, the context's resident map
int lift_prepare(mc_ctx *c, Pool &pool, const mc_contig_table *t1, const mc_contig_table *t2, LiftDev *T) {
    hipStream_t st = c->stream;
    *T = LiftDev();
    T->map = c->xmfa.map; T->n1 = c->xmfa.n1; T->nc1 = t1->n_contigs; T->nc2 = t2->n_contigs;
    if (int rc = lift_upload(pool, st, t1, &T->ids1, &T->id_off1, &T->off1)) return rc;
    if (int rc = lift_upload(pool, st, t2, &T->ids2, &T->id_off2, &T->off2)) return rc;
    T->cmask = table_slots(T->nc1, 64) - 1;
    unsigned long long *table = nullptr;
    if (int rc = table_get(pool, st, &table, T->cmask + 1)) return rc;
    T->ctable = table;
    if (T->nc1 > 0) hipLaunchKernelGGL(kc_contigs, dim3(blocks(T->nc1)), dim3(256), 0, st, *T, table, cmp_hash_mask());
    HIP_TRY(hipGetLastError());
    return 0;
}

bool lift_tables_ok(const mc_contig_table *t) {
    if (!t || t->n_contigs < 0 || !t->id_off || !t->off || (t->id_off[t->n_contigs] > 0 && !t->ids) || t->id_off[0] != 0 || t->off[0] != 0) return false;
    for (int64_t i = 0; i < t->n_contigs; ++i)
        if (t->id_off[i + 1] < t->id_off[i] || t->id_off[i + 1] - t->id_off[i] > 65535 || t->off[i + 1] < t->off[i]) return false;
    return true;
}

int cmp_call(mc_ctx *c, const mc_text_source &s1, const mc_text_source &s2, const char **out, int64_t *n_out, int64_t *n_sites, int32_t *status,
             const mc_contig_table *t1 = nullptr, const mc_contig_table *t2 = nullptr, const mc_cmp_options *opt = nullptr) {
    mc_cmp_stats &S = c->cmp.stats;
    return pipeline_call(c, S, status, "bed comparison", (size_t)32 << 20, [&] { *out = nullptr; *n_out = 0; *n_sites = 0; }, [&](Call &K) -> int {
        c->cmp.unaligned = 0;
        S.n_bytes1 = s1.n_bytes; S.n_bytes2 = s2.n_bytes;
        if (!cmp_fits((size_t)(s1.n_bytes + s2.n_bytes) + 4096)) return cmp_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
        char *d_text = nullptr;
        int64_t off2 = 0;
        if (K.pool.get(&d_text, (size_t)(s1.n_bytes + s2.n_bytes) + 1 + 64)) return -10;
        if (int rc = K.feed.put_pair(s1, &s2, d_text, &off2)) return rc;
        K.feed.times(S, K.t0);
        const auto t_kernels = std::chrono::steady_clock::now();
        LiftDev lift;
        int rc = t1 ? lift_prepare(c, K.pool, t1, t2, &lift) : 0;
        if (rc == 0) rc = cmp_run(c, K.pool, d_text, off2 + s2.n_bytes, off2, out, n_out, n_sites, status, t1 ? &lift : nullptr, opt);
        S.ms_kernels = ms_since(t_kernels) - S.ms_d2h;        // a declined call too: what ran until it declined
        return rc;
    });
}

}  // namespace

// the arguments of a lifted comparison beyond those of a plain one -> 0, or -12 with the error set
static int lifted_arguments(mc_ctx *c, const mc_contig_table *t1, const mc_contig_table *t2, int64_t *n_unaligned) {
    if (!n_unaligned || !lift_tables_ok(t1) || !lift_tables_ok(t2)) { mc_set_error("mc_bed_compare: bad arguments"); return -12; }
    if (!c->xmfa.map) { mc_set_error("mc_bed_compare: no alignment map is resident (mc_xmfa_map first)"); return -12; }
    if (t1->off[t1->n_contigs] != c->xmfa.n1 || t2->off[t2->n_contigs] != c->xmfa.n2) {
        mc_set_error("mc_bed_compare: the contig tables' totals are not those the map was built for");
        return -12;
    }
    return 0;
}

// opt: null, or the columns behind nlp_ks (mc_cmpfdr.inc)
extern "C" int mc_bed_compare_with(mc_ctx *c, const mc_text_source *bed1, const mc_text_source *bed2, const mc_contig_table *t1,
                                   const mc_contig_table *t2, const mc_cmp_options *opt, const char **out, int64_t *n_out, int64_t *n_sites,
                                   int64_t *n_unaligned, int32_t *status) {
    if (!c || !out || !n_out || !n_sites || !status || !t1 != !t2) {
        mc_set_error("mc_bed_compare: bad arguments");
        return -12;
    }
    if (n_unaligned) *n_unaligned = 0;
    if (t1)
        if (int rc = lifted_arguments(c, t1, t2, n_unaligned)) return rc;
    mc_text_source s1 = {}, s2 = {};
    if (int rc = text_source("mc_bed_compare", bed1, &s1)) return rc;
    if (int rc = text_source("mc_bed_compare", bed2, &s2)) return rc;
    const int rc = cmp_call(c, s1, s2, out, n_out, n_sites, status, t1, t2, opt);
    if (t1 && rc == 0 && *status == 0) *n_unaligned = c->cmp.unaligned;
    return rc;
}

extern "C" int mc_bed_compare(mc_ctx *c, const mc_text_source *bed1, const mc_text_source *bed2, const mc_contig_table *t1,
                              const mc_contig_table *t2, const char **out, int64_t *n_out, int64_t *n_sites, int64_t *n_unaligned,
                              int32_t *status) {
    return mc_bed_compare_with(c, bed1, bed2, t1, t2, nullptr, out, n_out, n_sites, n_unaligned, status);
}

extern "C" int mc_xmfa_map(mc_ctx *c, const mc_text_source *src, int32_t seq1, int32_t seq2, int64_t n1, int64_t n2, mc_xmfa_map_view *view,
                           int32_t *status) {
    if (!c || !status || n1 < 0 || n2 < 0 || seq1 == seq2) { mc_set_error("mc_xmfa_map: bad arguments"); return -12; }
    mc_text_source s = {};
    if (int rc = text_source("mc_xmfa_map", src, &s)) return rc;
    return xm_call(c, s, seq1, seq2, n1, n2, view, status);
}

extern "C" int mc_xmfa_map_last_stats(mc_ctx *c, mc_xmfa_stats *out) {
    return stats_out("mc_xmfa_map_last_stats", c, out, &mc_ctx::xmfa, &XmfaPipe::stats);
}

extern "C" int mc_xmfa_map_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::xmfa); }

extern "C" int mc_bed_compare_last_stats(mc_ctx *c, mc_cmp_stats *out) {
    return stats_out("mc_bed_compare_last_stats", c, out, &mc_ctx::cmp, &CmpPipe::stats);
}

extern "C" int mc_bed_compare_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::cmp); }

// a native sample against a control, site by site (mc_curcompare.inc)
extern "C" int mc_currents_compare(mc_ctx *c, const mc_text_source *native, const mc_text_source *control, const mc_cur_options *opt,
                                   mc_cur_result *res, int32_t *status) {
    if (!c || !opt || !res || !status || opt->depth < 2 || opt->by < -1 || opt->by > 3 || opt->n_columns < 0 || opt->n_columns > 65535 ||
        !(opt->log10c >= 0.0) || !(opt->log10c < 16.0) || !(opt->threshold == opt->threshold)) {
        mc_set_error("mc_currents_compare: bad arguments");
        return -12;
    }
    mc_text_source s1 = {}, s2 = {};
    if (int rc = text_source("mc_currents_compare", native, &s1)) return rc;
    if (int rc = text_source("mc_currents_compare", control, &s2)) return rc;
    return cur_call(c, s1, s2, *opt, res, status);
}

extern "C" int mc_currents_compare_last_stats(mc_ctx *c, mc_cur_stats *out) {
    return stats_out("mc_currents_compare_last_stats", c, out, &mc_ctx::currents, &CurPipe::stats);
}

extern "C" int mc_currents_compare_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::currents); }

// the rows of a sample's sites split in two by their currents (mc_sitecluster.inc)
extern "C" int mc_sites_cluster(mc_ctx *c, const mc_text_source *source, const mc_clu_options *opt, mc_clu_result *res, int32_t *status) {
    if (!c || !opt || !res || !status || opt->depth < 2 || opt->max_depth < 2 || opt->max_depth > MC_CLU_MAX_DEPTH ||
        (opt->metric != MC_CLU_CORRELATION && opt->metric != MC_CLU_EUCLIDEAN) || opt->n_columns < 0 || opt->n_columns > 65535 ||
        !(opt->min_minor == opt->min_minor) || !(opt->min_gap == opt->min_gap)) {
        mc_set_error("mc_sites_cluster: bad arguments");
        return -12;
    }
    mc_text_source src = {};
    if (int rc = text_source("mc_sites_cluster", source, &src)) return rc;
    return clu_call(c, src, *opt, res, status);
}

extern "C" int mc_sites_cluster_last_stats(mc_ctx *c, mc_clu_stats *out) {
    return stats_out("mc_sites_cluster_last_stats", c, out, &mc_ctx::clusters, &CluPipe::stats);
}

extern "C" int mc_sites_cluster_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::clusters); }

// methylation linkage between a sample's sites along its reads (mc_readphase.inc)
extern "C" int mc_reads_phase(mc_ctx *c, const mc_text_source *source, const mc_phase_options *opt, mc_phase_result *res, int32_t *status) {
    if (!c || !opt || !res || !status || opt->depth < 1 || opt->max_dist < 1 || opt->min_reads < 1 || opt->min_margin < 1 || opt->n_columns < 0 ||
        opt->n_columns > 65535 || !(opt->threshold == opt->threshold)) {
        mc_set_error("mc_reads_phase: bad arguments");
        return -12;
    }
    mc_text_source src = {};
    if (int rc = text_source("mc_reads_phase", source, &src)) return rc;
    return ph_call(c, src, *opt, res, status);
}

extern "C" int mc_reads_phase_last_stats(mc_ctx *c, mc_phase_stats *out) {
    return stats_out("mc_reads_phase_last_stats", c, out, &mc_ctx::phase, &PhasePipe::stats);
}

extern "C" int mc_reads_phase_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::phase); }

// the device build of mc_twosample.h on k sites: the rank kernels and kc_finish as the file pipeline runs them
extern "C" int mc_twosample_device(mc_ctx *c, const double *x, const int64_t *x_off, const double *y, const int64_t *y_off, int64_t k,
                                   double *out, double *bound, int32_t *status) {
    if (!c || !x || !x_off || !y || !y_off || k < 0 || (k > 0 && (!out || !bound || !status))) {
        mc_set_error("mc_twosample_device: bad arguments");
        return -12;
    }
    if (k == 0) return 0;
    for (int64_t i = 0; i < k; ++i)
        if (x_off[i + 1] < x_off[i] || y_off[i + 1] < y_off[i] || x_off[0] != 0 || y_off[0] != 0) {
            mc_set_error("mc_twosample_device: offsets that do not rise from 0");
            return -12;
        }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    Pool pool("two-sample batch");
    const size_t nk = (size_t)k, nx = (size_t)x_off[k], ny = (size_t)y_off[k];
    std::vector<long long> cnt(4 * nk);
    for (size_t i = 0; i < nk; ++i) {
        cnt[i] = x_off[i]; cnt[nk + i] = x_off[i + 1] - x_off[i];
        cnt[2 * nk + i] = y_off[i]; cnt[3 * nk + i] = y_off[i + 1] - y_off[i];
    }
    double *d_x = nullptr, *d_y = nullptr, *d_out = nullptr, *d_bound = nullptr;
    long long *d_cnt = nullptr;
    unsigned long long *d_n = nullptr;
    TwSite *d_sites = nullptr;
    int32_t *d_status = nullptr;
    if (pool.get(&d_x, nx + 1) || pool.get(&d_y, ny + 1) || pool.get(&d_cnt, 4 * nk) || pool.get(&d_n, 2) || pool.get(&d_sites, nk) ||
        pool.get(&d_out, nk * TW_N_OUT) || pool.get(&d_bound, nk * TW_N_OUT) || pool.get(&d_status, nk))
        return -10;
    if (nx) HIP_TRY(hipMemcpyAsync(d_x, x, nx * 8, hipMemcpyHostToDevice, st));
    if (ny) HIP_TRY(hipMemcpyAsync(d_y, y, ny * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cnt, cnt.data(), 4 * nk * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_n, 0, 16, st));
    HIP_TRY(hipMemsetAsync(d_sites, 0, nk * sizeof(TwSite), st));
    RankArgs R = {d_x, d_y, d_cnt, d_cnt + nk, d_cnt + 2 * nk, d_cnt + 3 * nk, k, d_sites, d_n, d_n + 1};
    int rc = launch_ranks(st, R);
    if (rc == 0) {
        hipLaunchKernelGGL(kc_finish, dim3(blocks(k)), dim3(256), 0, st, (const TwSite *)d_sites, (const long long *)(d_cnt + nk),
                           (const long long *)(d_cnt + 3 * nk), k, d_out, d_bound, d_status, (double *)nullptr, (double *)nullptr);
        rc = mc_hip_rc(hipGetLastError(), "kc_finish");
    }
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(out, d_out, nk * TW_N_OUT * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(bound, d_bound, nk * TW_N_OUT * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(status, d_status, nk * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    const int rc_sync = mc_hip_rc(hipStreamSynchronize(st), "hipStreamSynchronize");      // (nothing of the pool is in use when it goes)
    return rc ? rc : rc_sync;
}

// mc_fisher.h's device build on `count` tables, a lane per table (mc_cmpfdr.inc)
extern "C" int mc_fisher_exact_device(mc_ctx *c, const int64_t *K1, const int64_t *n1, const int64_t *K2, const int64_t *n2, int64_t count,
                                      double *log10_p, double *bound, int32_t *status) {
    if (!c || count < 0 || (count > 0 && (!K1 || !n1 || !K2 || !n2 || !log10_p || !bound || !status))) {
        mc_set_error("mc_fisher_exact_device: bad arguments");
        return -12;
    }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return fisher_batch(c, K1, n1, K2, n2, count, log10_p, bound, status);
}

// the Benjamini-Hochberg adjustment of one column on the device (mc_cmpfdr.inc)
extern "C" int mc_bh_adjust_device(mc_ctx *c, const double *L, const double *bound, int64_t n, double *Q, double *rounded, int32_t *status) {
    if (!c || n < 0 || n > 2147483646LL || !status || (n > 0 && (!L || !bound || !Q || !rounded))) {
        mc_set_error("mc_bh_adjust_device: bad arguments");
        return -12;
    }
    *status = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return fdr_adjust(c, L, bound, n, Q, rounded, status);
}
