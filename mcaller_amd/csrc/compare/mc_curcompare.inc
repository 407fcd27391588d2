// mc_curcompare.inc -- a native sample against an unmodified control, site by site and WITHOUT a model: the rows of
// compare_currents.compare_currents made on the GPU from the texts of two .diffs files (C ABI: mc_currents_compare,
// mc_currents_compare_last_stats, mc_currents_compare_release; Python: Device.currents_compare,
// compare_currents.compare_currents_device).  Part of the mc_bedcompare.hip unit, included behind mc_cmpfdr.inc: it shares the unit's
// helpers and calls kc_rank_small, both kc_rank_large instances, kc_finish and kc_fdr_* (fdr_column) as they are; its own kernels are kn_*.
//
// The result is the host statement's bytes or a decline (status 1, mc_last_error; the stats say which file and line).  The reasons of
// mc_bedcompare.hip where they apply -- MC_CMP_DECLINE_HIGH_BYTE, _CONTROL, _LONG_LINE, _ROWS, _MEMORY, _TABLE, _NUMBER (a value, the
// read quality included, on any line of either file), _DEPTH (more than TW_MAX_N pooled values in a column; the site's first native line
// is named), _NAN, _ALL_EQUAL, _FAR_TAIL, _PRINT, _TIE (a site's value: its first native line; a q-value: no line) -- and three of its own:
//   MC_CMP_DECLINE_CUR_FIELDS   a line that does not have 7 or 8 tab-separated fields (the host's ValueError)
//   MC_CMP_DECLINE_CUR_VALUES   a line whose number of values is not the caller's n_columns + 1, or fewer than 2 (the host's ValueError)
//   MC_CMP_DECLINE_CUR_POS      a pos that is not 1 .. 9 plain digits without a leading zero (int() may take it: the host decides)
//
// The two texts stand behind one another in one device buffer (mc_textfeed.h; a '\n' between them when the native text's last line has
// none); a line is native when it starts before the control's text.  The steps (L lines, S kept sites, c columns, R rows of kept sites):
//   kp_count / kp_scan / kp_starts   line starts (mc_lines.h)
//   kn_parse     a lane per line, 256 lines of a workgroup staged in LDS (staged_lines): ByteClass, the 6 or 7 tabs, the KeyHash of
//                chrom, pos and strand, the comma count, every number's grammar (mc_decimal.h: the host calls float() on all of
//                them), the plain-digit test of pos
//   kn_group     ONE key table for both files (kt_claim, byte comparison).  The line that claimed the slot names the key; per key the
//                smallest native line (atomicMin) and the rows of each file (atomicAdd), integers all: nothing depends on arrival
//   kn_select / kp_scan   a key is kept where it has -d rows in both files; its smallest native line is its head.  The scan over
//                the head flags numbers the kept sites in the order of their first native rows (no atomic decides an order)
//   kn_sites / kp_scan x 2   per site: head line, rows per file; the samples' row offsets
//   kn_claim / kn_place   rows into their (site, file) bucket in arrival order (atomicAdd), then every row's RANK among its
//                bucket's line numbers -> the bucket in ascending line order: what the later kernels read does not depend on arrival.
//                A lane per row reads its bucket once: linear in the depth per row
//   kn_pseudo    (site, column) = one pseudo-site of RankArgs: offsets and counts into column-major arrays
//   kn_values    a lane per NUMBER: mc_decimal.h -> x and y, (site, column) one contiguous run each
//   kc_rank_small / kc_rank_large x 2 / kc_finish   over the S c pseudo-sites, unchanged
//   kn_combine   a lane per site: every column's status, the t_j, mc_curcombine.h per test -> L, its bound, the printed nlp
//   kc_fdr_*     (--fdr) fdr_column once per test over the S combined L
//   kn_size / kp_scan x 2 / kn_write   per site the row's and the bed line's length (the --sig_bed decision on the PRINTED value),
//                their places, their bytes (mc_rowtext.h); two outputs
// No floating-point atomic anywhere.
// Resources (tools/kres.py, gfx950; none spills or uses scratch; the kc_* figures of mc_bedcompare.hip's header stand as they were):
//   kn_parse    44 VGPRs, 48 KB + 16 bytes of dynamic LDS (the staged lines: three workgroups a CU of its 160 KB), 8 waves a SIMD by registers
//   kn_group    41 VGPRs    kn_values   42    kn_size  54    kn_write  64 (the digit generation of mc_rowtext.h)    kn_combine  30
//   kn_select   10    kn_sites  14    kn_claim  10    kn_place  12    kn_pseudo  18
//   none uses static LDS; every one runs at 8 waves a SIMD.  kn_place is the one kernel whose work is not linear in the file: a lane
//   reads its bucket once, n1^2 + n2^2 reads a site -- 2^25 at the depth cap, beside kc_rank_large's 2^26 compares of the same site
// Measured (MI355X, tools/currents_probe.py, profiles/currents_probe.json and profiles/currents_kernel_stats.csv; synthetic `-m A`-like
// pairs of depth 15 .. 60 with six columns, --fdr --sig_bed, file to file, medians of 3, files in the page cache):
//   2000 sites / 12.5 MB    15.9 s -> 0.0047 s (x3400 against the host statement on the same box, 1.32 ms a site and column; the
//                           device's rows and bed equal the host's); kernels 2.0 ms, of which the four q-value columns 0.77 ms
//   20000 sites / 127 MB    0.0183 s on the device (kernels 6.8 ms, the files' way from the page cache 5.8 ms); the host was not timed
//   a run of 2000 sites, by kernel: kn_parse 0.138 ms, kc_rank_large<512> 0.123, kc_finish 0.105, kn_write 0.073, kc_rank_small 0.060,
//   kn_group 0.054, kn_values 0.052, kn_size 0.051, kn_place 0.030, kn_combine 0.015, kn_claim 0.015, kn_pseudo / kn_select / kn_sites
//   0.005 each: the eleven kn_* are 0.44 ms of 1.63 ms, the q-values' sorts (32 kc_fdr_place and kc_fdr_count) and the 38 single-
//   workgroup kp_scan take as much again.  Not measured: other depths and column counts, files that are not in the page cache.
#include "../mc_curcombine.h"

constexpr int CU_STAGE = 48 * 1024;          // LDS a workgroup of kn_parse stages its 256 lines in (as kb_parse)
constexpr unsigned CU_NONE = 0xffffffffu;

struct CurHead {                             // device-side result block (copied to the host as it is)
    KpHead kp;
    unsigned long long decline;              // min over the offending lines of line << 8 | reason (~0: none)
    long long n_lines1;                      // lines that start before the control's text
    long long n_sites, n_rx, n_ry, out_bytes, bed_bytes;      // totals of the scans
    unsigned long long n_small, n_large;     // pseudo-sites each rank kernel took
    unsigned long long n_sig, n_keys;
    int longest_probe, deepest;
};

struct CurArgs {
    const char *text;
    int64_t n_bytes, off2, n_nl, n_lines, n_lines1;
    const long long *line_start;
    CurHead *head;
    int depth, c, fdr, by;                   // by: 0 .. 3, -1: no bed
    double log10c, threshold;
    // per line
    uint4 *span;                             // tabs_pack (t6 = len in a 7-field row); 0: not a line the table takes
    uint64_t *hash;
    uint32_t *n_vals, *rep;                  // rep: the line that names the line's key
    long long *flag, *site_of;               // native lines: 1 at a kept site's head, the scan
    uint64_t hash_mask, mask;
    unsigned long long *table;
    // per key, at the line that names it
    uint32_t *key_first, *key_cnt;           // smallest native line; rows of the native file [rep], of the control [cap + rep]
    int32_t *key_site;                       // the kept site's number, -1: none
    int64_t cap;
    // per site
    int64_t S;
    long long *head_line, *cnt1, *cnt2, *off1, *off2r, *row_len, *row_off, *bed_len, *bed_off;
    unsigned int *fill;                      // [2 S]
    // per row of a kept site: native rows [0, n_rx), control rows [n_rx, n_rx + n_ry)
    int64_t n_rx, n_ry;
    uint32_t *claimed, *rows;                // line numbers in arrival order, in ascending order
    // per pseudo-site (site, column)
    long long *p_xoff, *p_xcnt, *p_yoff, *p_ycnt;
    double *vals;                            // x[0, c n_rx) then y[0, c n_ry)
    TwSite *sites;
    double *out9, *bound9, *logs, *log_bound;
    int32_t *status;
    // per site: the four combined L, their bounds, the printed nlp, the printed nlq
    double *comb, *comb_bound, *nlp, *nlq;
    char *out, *bed;
};

__device__ __forceinline__ TabSpan cu_line(const CurArgs &A, int64_t li) { return tabs_unpack(A.span[li]); }

// One line: t[x - adj] is byte x of the text (the staged piece in LDS, or the text itself with adj = 0)
__device__ __forceinline__ void cu_parse_line(const CurArgs &A, const char *t, const int64_t adj, const int64_t li) {
    const int64_t b = A.line_start[li] - adj;
    const int64_t e = (li < A.n_nl ? A.line_start[li + 1] - 1 : A.n_bytes) - adj;
    A.span[li] = make_uint4(0u, 0u, 0u, 0u);
    A.hash[li] = 0;
    A.n_vals[li] = 0;
    A.rep[li] = CU_NONE;
    if (b + adj < A.off2 && (li + 1 >= A.n_lines || (int64_t)A.line_start[li + 1] >= A.off2)) A.head->n_lines1 = li + 1;      // the native text's last line alone
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_LONG_LINE); return; }
    const int len = (int)(e - b);
    int tab[7] = {0, 0, 0, 0, 0, 0, 0}, nt = 0, commas = 0;
    ByteClass bad;
    KeyHash H;
    for (int i = 0; i < len; ++i) {
        const unsigned ch = (unsigned char)t[b + i];
        bad.see(ch);
        if (ch == '\t') {
#pragma unroll
            for (int k = 0; k < 7; ++k) tab[k] = nt == k ? i : tab[k];
            if (nt == 0 || nt == 2) H.sep();                          // behind chrom, behind pos
            ++nt;
        } else if (nt == 0 || nt == 2 || nt == 5) {                   // chrom, pos, strand
            H.put((char)ch);
        } else if (nt == 4) {
            commas += ch == ',';
        }
    }
    if (bad.hi) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CONTROL); return; }
    if (nt != 6 && nt != 7) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CUR_FIELDS); return; }
    if (nt == 6) tab[6] = len;
    // every number of the line, the read quality too: the host calls float() on all of them
    bool bad_number = false;
    for (int p = tab[3] + 1, tb = tab[3] + 1; p <= tab[4]; ++p)
        if (p == tab[4] || t[b + p] == ',') {
            double d;
            bad_number |= !dc_parse(t + b + tb, p - tb, &d);
            tb = p + 1;
        }
    if (bad_number) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_NUMBER); return; }
    if (commas + 1 != A.c + 1 || A.c < 1) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CUR_VALUES); return; }
    const int pn = tab[2] - tab[1] - 1;
    bool plain = pn >= 1 && pn <= 9 && !(pn > 1 && t[b + tab[1] + 1] == '0');
    for (int i = tab[1] + 1; i < tab[2]; ++i) plain = plain && (unsigned)((unsigned char)t[b + i]) - '0' <= 9u;
    if (!plain) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CUR_POS); return; }
    A.hash[li] = H.done(A.hash_mask);
    A.n_vals[li] = (uint32_t)commas + 1u;
    A.span[li] = tabs_pack(tab, len);
}

__global__ __launch_bounds__(256) void kn_parse(CurArgs A) {
    (void)staged_lines<CU_STAGE>(A.text, A.n_bytes, A.line_start, A.n_lines, A.n_nl,
                                 [&](const char *t, int64_t adj, int64_t li) { cu_parse_line(A, t, adj, li); });
}

// (chrom, pos, strand) of lines a and b, byte for byte
__device__ __forceinline__ bool cu_same_key(const CurArgs &A, int64_t a, int64_t b) {
    const TabSpan La = cu_line(A, a), Lb = cu_line(A, b);
    if (La.t[0] != Lb.t[0] || La.t[2] - La.t[1] != Lb.t[2] - Lb.t[1] || La.t[5] - La.t[4] != Lb.t[5] - Lb.t[4]) return false;
    const char *pa = A.text + A.line_start[a], *pb = A.text + A.line_start[b];
    return same_bytes(pa, pb, La.t[0]) && same_bytes(pa + La.t[1] + 1, pb + Lb.t[1] + 1, La.t[2] - La.t[1] - 1) &&
           same_bytes(pa + La.t[4] + 1, pb + Lb.t[4] + 1, La.t[5] - La.t[4] - 1);
}

__global__ __launch_bounds__(256) void kn_group(CurArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines || cu_line(A, li).len == 0) return;            // (a line kn_parse left out: it has declined the file)
    const uint64_t h = A.hash[li];
    const KtHit hit = kt_claim(A.table, A.mask, h, li, [&](int64_t r) { return A.hash[r] == h && cu_same_key(A, li, r); });
    if (hit.slot < 0 || hit.id < 0 || hit.id >= A.n_lines) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_TABLE); return; }
    const int64_t rep = hit.id;
    A.rep[li] = (uint32_t)rep;
    const bool native = li < A.n_lines1;
    atomicAdd(&A.key_cnt[(native ? 0 : A.cap) + rep], 1u);
    if (native) atomicMin(&A.key_first[rep], (uint32_t)li);
    if (hit.claimed) atomicAdd(&A.head->n_keys, 1ull);
    const int looked = (int)(hit.looked > 0x7fffffffull ? 0x7fffffffull : hit.looked);
    if (looked > A.head->longest_probe) atomicMax(&A.head->longest_probe, looked);
}

// a native line is the head of a kept site: the smallest native line of a key with -d rows in both files
__global__ __launch_bounds__(256) void kn_select(CurArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1) return;
    long long keep = 0;
    const uint32_t rep = A.rep[li];
    if (rep != CU_NONE && A.key_first[rep] == (uint32_t)li) {
        const long long c1 = A.key_cnt[rep], c2 = A.key_cnt[A.cap + rep];
        if (c1 >= A.depth && c2 >= A.depth) {
            keep = 1;
            if (c1 + c2 > TW_MAX_N) line_flag(&A.head->decline, li, MC_CMP_DECLINE_DEPTH);
            const int deep = (int)(c1 + c2 > 0x7fffffffll ? 0x7fffffffll : c1 + c2);
            if (deep > A.head->deepest) atomicMax(&A.head->deepest, deep);
        }
    }
    A.flag[li] = keep;
}

__global__ __launch_bounds__(256) void kn_sites(CurArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1 || A.flag[li] == 0) return;
    const long long s = A.site_of[li];
    if (s < 0 || s >= A.S) return;                                     // (cannot be: the scan counted these lines)
    const uint32_t rep = A.rep[li];
    A.head_line[s] = li;
    A.cnt1[s] = A.key_cnt[rep]; A.cnt2[s] = A.key_cnt[A.cap + rep];
    A.key_site[rep] = (int32_t)s;
}

// the site of line li (-1: its key is not kept), which file it is of, where its bucket starts and how many rows it has
struct CuRow { long long s, off, n; bool control; };
__device__ __forceinline__ CuRow cu_row(const CurArgs &A, int64_t li) {
    CuRow r{-1, 0, 0, li >= A.n_lines1};
    const uint32_t rep = A.rep[li];
    if (rep == CU_NONE) return r;
    const long long s = A.key_site[rep];
    if (s < 0 || s >= A.S) return r;
    r.s = s;
    r.off = r.control ? A.n_rx + A.off2r[s] : A.off1[s];
    r.n = r.control ? A.cnt2[s] : A.cnt1[s];
    return r;
}

__global__ __launch_bounds__(256) void kn_claim(CurArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines) return;
    const CuRow r = cu_row(A, li);
    if (r.s < 0) return;
    const long long k = atomicAdd(&A.fill[2 * r.s + (r.control ? 1 : 0)], 1u);
    if (k < r.n && r.off + k < A.n_rx + A.n_ry) A.claimed[r.off + k] = (uint32_t)li;      // (always: the counts are kn_group's)
}

// the rank of a row's line number among its bucket's: its place in ascending line order
__global__ __launch_bounds__(256) void kn_place(CurArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines) return;
    const CuRow r = cu_row(A, li);
    if (r.s < 0 || r.off + r.n > A.n_rx + A.n_ry) return;
    long long rank = 0;
    for (long long k = 0; k < r.n; ++k) rank += A.claimed[r.off + k] < (uint32_t)li;
    A.rows[r.off + rank] = (uint32_t)li;
}

__global__ __launch_bounds__(256) void kn_pseudo(CurArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.S * A.c) return;
    const int64_t s = p / A.c, j = p % A.c;
    A.p_xoff[p] = A.c * A.off1[s] + j * A.cnt1[s]; A.p_xcnt[p] = A.cnt1[s];
    A.p_yoff[p] = A.c * A.off2r[s] + j * A.cnt2[s]; A.p_ycnt[p] = A.cnt2[s];
}

// a lane per NUMBER: value j of the row at place r -> the column-major arrays
__global__ __launch_bounds__(256) void kn_values(CurArgs A) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (A.n_rx + A.n_ry) * A.c) return;
    const int64_t r = v / A.c;
    const int j = (int)(v % A.c);
    const int64_t li = A.rows[r];
    if (li >= A.n_lines) return;
    const CuRow R = cu_row(A, li);
    if (R.s < 0) return;
    const long long place = r - R.off;
    if (place < 0 || place >= R.n) return;
    const TabSpan L = cu_line(A, li);
    const char *t = A.text + A.line_start[li];
    int tb = L.t[3] + 1, k = 0, p = L.t[3] + 1;
    for (; p < L.t[4]; ++p)
        if (t[p] == ',') {
            if (k == j) break;
            ++k; tb = p + 1;
        }
    double d = 0.0;
    if (k != j || !dc_parse(t + tb, p - tb, &d)) line_flag(&A.head->decline, li, MC_CMP_DECLINE_NUMBER);
    const long long base = R.control ? A.c * A.n_rx + A.c * A.off2r[R.s] : A.c * A.off1[R.s];
    A.vals[base + (long long)j * R.n + place] = d;
}

__device__ __forceinline__ int cu_tw_reason(int st) {
    return (st & TW_ALL_EQUAL) ? MC_CMP_DECLINE_ALL_EQUAL : (st & (TW_BAD_N | TW_ZERO_VAR)) ? MC_CMP_DECLINE_NAN
         : (st & TW_DEEP) ? MC_CMP_DECLINE_DEPTH : (st & TW_FAR_TAIL) ? MC_CMP_DECLINE_FAR_TAIL
         : (st & TW_UNPRINTABLE) ? MC_CMP_DECLINE_PRINT : MC_CMP_DECLINE_TIE;
}

// a lane per site: its columns' status, then the four tests' columns into one L each (mc_curcombine.h)
__global__ __launch_bounds__(256) void kn_combine(CurArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    const double nan = __builtin_nan("");
    for (int i = 0; i < 4; ++i) { A.comb[s * 4 + i] = nan; A.comb_bound[s * 4 + i] = 0.0; A.nlp[s * 4 + i] = nan; }
    int st = 0;
    for (int j = 0; j < A.c; ++j) st |= A.status[s * A.c + j];
    if (st) { line_flag(&A.head->decline, A.head_line[s], cu_tw_reason(st)); return; }
    for (int i = 0; i < 4; ++i) {
        CcMin M;
        for (int j = 0; j < A.c; ++j) M.column(A.logs[(s * A.c + j) * CMP_LOGS + i], A.log_bound[(s * A.c + j) * CMP_LOGS + i]);
        double L, b, rounded;
        const int cc = M.finish(A.log10c, &L, &b, &rounded);
        if (cc) {
            const int reason = (cc & CC_NAN) ? MC_CMP_DECLINE_NAN : (cc & CC_RANGE) ? MC_CMP_DECLINE_FAR_TAIL
                             : (cc & CC_UNPRINTABLE) ? MC_CMP_DECLINE_PRINT : MC_CMP_DECLINE_TIE;
            line_flag(&A.head->decline, A.head_line[s], reason);
            continue;
        }
        A.comb[s * 4 + i] = L; A.comb_bound[s * 4 + i] = b; A.nlp[s * 4 + i] = rounded;
    }
}

__device__ __forceinline__ uint32_t cu_pos(const char *p, const TabSpan &L) {
    uint32_t pos = 0;
    for (int i = L.t[1] + 1; i < L.t[2]; ++i) pos = pos * 10u + (uint32_t)(p[i] - '0');
    return pos;
}

// the printed value --sig_bed goes by
__device__ __forceinline__ double cu_sig_value(const CurArgs &A, int64_t s) { return (A.fdr ? A.nlq : A.nlp)[s * 4 + A.by]; }

template <class Sink>
__device__ __forceinline__ void cu_put_row(const CurArgs &A, int64_t s, Sink &o) {
    const long long li = A.head_line[s];
    const TabSpan L = cu_line(A, li);
    const char *p = A.text + A.line_start[li];
    for (int i = 0; i <= L.t[0]; ++i) o.put(p[i]);                     // chrom and its tab
    for (int i = L.t[1] + 1; i <= L.t[2]; ++i) o.put(p[i]);            // pos
    rt_put_uint(o, cu_pos(p, L) + 1u); o.put('\t');
    for (int i = L.t[2] + 1; i <= L.t[3]; ++i) o.put(p[i]);            // context
    for (int i = L.t[4] + 1; i <= L.t[5]; ++i) o.put(p[i]);            // strand
    rt_put_uint(o, (uint32_t)A.cnt1[s]); o.put('\t');
    rt_put_uint(o, (uint32_t)A.cnt2[s]); o.put('\t');
    for (int j = 0; j < A.c; ++j) { rt_put_num(o, rt_num_of(A.out9[(s * A.c + j) * TW_N_OUT + 3])); o.put('\t'); }
    for (int i = 0; i < 4; ++i) { rt_put_num(o, rt_num_of(A.nlp[s * 4 + i])); o.put(i < 3 || A.fdr ? '\t' : '\n'); }
    if (A.fdr)
        for (int i = 0; i < 4; ++i) { rt_put_num(o, rt_num_of(A.nlq[s * 4 + i])); o.put(i < 3 ? '\t' : '\n'); }
}

// chrom pos pos+1 context nlp strand n_native
template <class Sink>
__device__ __forceinline__ void cu_put_bed(const CurArgs &A, int64_t s, Sink &o) {
    const long long li = A.head_line[s];
    const TabSpan L = cu_line(A, li);
    const char *p = A.text + A.line_start[li];
    for (int i = 0; i <= L.t[0]; ++i) o.put(p[i]);
    for (int i = L.t[1] + 1; i <= L.t[2]; ++i) o.put(p[i]);
    rt_put_uint(o, cu_pos(p, L) + 1u); o.put('\t');
    for (int i = L.t[2] + 1; i <= L.t[3]; ++i) o.put(p[i]);
    rt_put_num(o, rt_num_of(cu_sig_value(A, s))); o.put('\t');
    for (int i = L.t[4] + 1; i <= L.t[5]; ++i) o.put(p[i]);
    rt_put_uint(o, (uint32_t)A.cnt1[s]); o.put('\n');
}

__global__ __launch_bounds__(256) void kn_size(CurArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool sig = false;
    if (s < A.S) {
        A.row_len[s] = 0; A.bed_len[s] = 0;
        bool ok = true;
        for (int i = 0; i < 4; ++i) {                                  // (a NaN: the site's line has declined the file with its own reason)
            const double v = A.nlp[s * 4 + i], q = A.fdr ? A.nlq[s * 4 + i] : 0.0;
            if (v != v || q != q) { ok = false; break; }
            if (!rt_num_of(v).ok || !rt_num_of(q).ok) { line_flag(&A.head->decline, A.head_line[s], MC_CMP_DECLINE_PRINT); ok = false; break; }
        }
        if (ok) {
            RtCount count;
            cu_put_row(A, s, count);
            A.row_len[s] = count.n;
            if (A.by >= 0 && cu_sig_value(A, s) >= A.threshold) {
                RtCount bed;
                cu_put_bed(A, s, bed);
                A.bed_len[s] = bed.n;
                sig = true;
            }
        }
    }
    const unsigned long long bal = __ballot(sig);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_sig, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(256) void kn_write(CurArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    const long long at = A.row_off[s], len = A.row_len[s];
    if (len > 0 && at >= 0 && at + len <= A.head->out_bytes) {         // (always: the scan counted these bytes)
        RtStore store{A.out + at};
        cu_put_row(A, s, store);
    }
    const long long bat = A.bed_off[s], blen = A.bed_len[s];
    if (blen > 0 && bat >= 0 && bat + blen <= A.head->bed_bytes) {
        RtStore store{A.bed + bat};
        cu_put_bed(A, s, store);
    }
}

const char *cur_reason_text(int reason) {
    switch (reason) {
        case MC_CMP_DECLINE_CUR_FIELDS: return "a line that does not have 7 or 8 tab-separated fields";
        case MC_CMP_DECLINE_CUR_VALUES: return "a line whose number of values is not that of the native file's first row, or fewer than 2";
        case MC_CMP_DECLINE_CUR_POS: return "a pos that is not plain digits";
        case MC_CMP_DECLINE_NUMBER: return "a value the device's decimal reader declines";
        case MC_CMP_DECLINE_DEPTH: return "a site with more than 8192 pooled values in a column";
        case MC_CMP_DECLINE_NAN: return "a column with fewer than 3 pooled values or a zero pooled variance";
        case MC_CMP_DECLINE_ALL_EQUAL: return "a column whose pooled values are all equal";
        case MC_CMP_DECLINE_FAR_TAIL: return "a log10 p below -290";
    }
    return cmp_reason_text(reason);
}

// file: 1 (native), 2 (control) or 0; line: in that file, -1: none
int cur_decline(mc_ctx *c, int32_t *status, int reason, int file, long long line) {
    c->cur_stats.decline_file = file;
    char what[200];
    if (file) snprintf(what, sizeof what, "%s (%s)", cur_reason_text(reason), file == 1 ? "native" : "control");
    else snprintf(what, sizeof what, "%s", cur_reason_text(reason));
    return decline(c->cur_stats, status, "current comparison", what, reason, line);
}

int cur_decline_head(mc_ctx *c, int32_t *status, const CurHead &h) {
    const long long line = decline_line(h.decline);
    const bool first = line < h.n_lines1;
    return cur_decline(c, status, decline_reason(h.decline), first ? 1 : 2, first ? line : line - h.n_lines1);
}

// one of the call's two outputs: device bytes -> the context's pinned block
int cur_fetch(mc_ctx *c, Pinned &dst, size_t &dst_cap, const char *d_src, size_t n, const char **out, int64_t *n_out) {
    *out = nullptr; *n_out = 0;
    if (n == 0) return 0;
    if (int rc = grow(dst, dst_cap, n)) return rc;
    HIP_TRY(hipMemcpyAsync(dst.p, d_src, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = dst.get<char>();
    *n_out = (int64_t)n;
    return 0;
}

// The texts are on the device (d_text[0, n): the native text, a newline if it lacked its last, the control's from off2 on; padded)
int cur_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, int64_t off2, const mc_cur_options &opt, mc_cur_result *res, int32_t *status) {
    mc_cur_stats &S = c->cur_stats;
    hipStream_t st = c->stream;
    if (n == 0) return 0;
    CurHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline = CMP_NO_DECLINE;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, d_text, n, &d_head->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t n_nl = h.kp.n_newlines;
    if (too_many_lines(n_nl)) return cur_decline(c, status, MC_CMP_DECLINE_ROWS, 0, -1);
    const size_t cap = (size_t)n_nl + 2;
    if (!cmp_fits(cap * (8 + 16 + 8 + 4 + 4 + 8 + 8 + 4 + 8 + 4) + ((size_t)1 << 20))) return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    if (int rc = lines_starts(pool, st, d_text, n, n_nl, tile_off, &d_head->kp, &line_start)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t L = h.kp.n_lines;
    if (L <= 0 || L > (int64_t)cap) return 0;
    CurArgs A = {};
    A.text = d_text; A.n_bytes = n; A.off2 = off2; A.n_nl = n_nl; A.n_lines = L; A.line_start = line_start; A.head = d_head;
    A.depth = opt.depth; A.c = opt.n_columns; A.fdr = opt.fdr != 0; A.by = opt.by; A.log10c = opt.log10c; A.threshold = opt.threshold;
    A.cap = (int64_t)cap;
    const char *hm = getenv("MCALLER_CMP_HASH_MASK");
    A.hash_mask = hm && *hm ? strtoull(hm, nullptr, 16) : ~0ull;      // (tests: long probe chains)
    if (pool.get(&A.span, cap) || pool.get(&A.hash, cap) || pool.get(&A.n_vals, cap) || pool.get(&A.rep, cap) || pool.get(&A.flag, cap) ||
        pool.get(&A.site_of, cap) || pool.get(&A.key_first, cap) || pool.get(&A.key_cnt, 2 * cap) || pool.get(&A.key_site, cap))
        return -10;
    hipLaunchKernelGGL(kn_parse, dim3(blocks(L)), dim3(256), CU_STAGE + 16, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t L1 = h.n_lines1, L2 = L - L1;
    S.n_lines1 = L1; S.n_lines2 = L2;
    if (h.decline != CMP_NO_DECLINE) return cur_decline_head(c, status, h);
    A.n_lines1 = L1;
    if (L1 == 0 || L2 == 0) return 0;
    A.mask = table_slots(L, 64, "MCALLER_CMP_TABLE_SLOTS") - 1;
    S.table_slots = (int64_t)A.mask + 1;
    if (!cmp_fits((A.mask + 1) * 8 + ((size_t)1 << 20))) return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    if (int rc = table_get(pool, st, &A.table, A.mask + 1)) return rc;
    HIP_TRY(hipMemsetAsync(A.key_first, 0xff, cap * 4, st));
    HIP_TRY(hipMemsetAsync(A.key_cnt, 0, 2 * cap * 4, st));
    HIP_TRY(hipMemsetAsync(A.key_site, 0xff, cap * 4, st));
    hipLaunchKernelGGL(kn_group, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kn_select, dim3(blocks(L1)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.flag, L1, A.site_of, &d_head->n_sites);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_keys = (int64_t)h.n_keys; S.longest_probe = h.longest_probe; S.deepest_site = h.deepest;
    if (h.decline != CMP_NO_DECLINE) return cur_decline_head(c, status, h);
    const int64_t NS = h.n_sites;
    S.n_sites = NS;
    if (NS <= 0) return 0;
    A.S = NS;
    const size_t ns = (size_t)NS, np = ns * (size_t)A.c;
    if (!cmp_fits(ns * (9 * 8 + 2 * 4 + 16 * 8) + np * (4 * 8 + sizeof(TwSite) + 2 * 8 * TW_N_OUT + 2 * 8 * CMP_LOGS + 4) + (A.fdr ? fdr_bytes(NS) : 0) +
                  ((size_t)1 << 20)))
        return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    if (pool.get(&A.head_line, ns) || pool.get(&A.cnt1, ns) || pool.get(&A.cnt2, ns) || pool.get(&A.off1, ns) || pool.get(&A.off2r, ns) ||
        pool.get(&A.row_len, ns) || pool.get(&A.row_off, ns) || pool.get(&A.bed_len, ns) || pool.get(&A.bed_off, ns) || pool.get(&A.fill, 2 * ns) ||
        pool.get(&A.p_xoff, np) || pool.get(&A.p_xcnt, np) || pool.get(&A.p_yoff, np) || pool.get(&A.p_ycnt, np) || pool.get(&A.sites, np) ||
        pool.get(&A.out9, np * TW_N_OUT) || pool.get(&A.bound9, np * TW_N_OUT) || pool.get(&A.logs, np * CMP_LOGS) ||
        pool.get(&A.log_bound, np * CMP_LOGS) || pool.get(&A.status, np) || pool.get(&A.comb, 4 * ns) || pool.get(&A.comb_bound, 4 * ns) ||
        pool.get(&A.nlp, 4 * ns) || pool.get(&A.nlq, 4 * ns))
        return -10;
    HIP_TRY(hipMemsetAsync(A.fill, 0, 2 * ns * 4, st));
    HIP_TRY(hipMemsetAsync(A.sites, 0, np * sizeof(TwSite), st));
    HIP_TRY(hipMemsetAsync(A.nlq, 0, 4 * ns * 8, st));
    hipLaunchKernelGGL(kn_sites, dim3(blocks(L1)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt1, NS, A.off1, &d_head->n_rx);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt2, NS, A.off2r, &d_head->n_ry);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    A.n_rx = h.n_rx; A.n_ry = h.n_ry;
    const size_t nr = (size_t)(h.n_rx + h.n_ry), nv = nr * (size_t)A.c;
    S.n_values = (int64_t)nv;
    if (!cmp_fits(nr * 8 + nv * 8 + ((size_t)1 << 20))) return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    if (pool.get(&A.claimed, nr + 1) || pool.get(&A.rows, nr + 1) || pool.get(&A.vals, nv + 1)) return -10;
    HIP_TRY(hipMemsetAsync(A.claimed, 0xff, (nr + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(A.rows, 0xff, (nr + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(A.vals, 0, (nv + 1) * 8, st));
    hipLaunchKernelGGL(kn_claim, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kn_place, dim3(blocks(L)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kn_pseudo, dim3(blocks((int64_t)np)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kn_values, dim3(blocks((int64_t)nv)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    RankArgs R = {A.vals, A.vals + (size_t)A.c * (size_t)A.n_rx, A.p_xoff, A.p_xcnt, A.p_yoff, A.p_ycnt, (int64_t)np, A.sites, &d_head->n_small,
                  &d_head->n_large};
    if (int rc = launch_ranks(st, R)) return rc;
    hipLaunchKernelGGL(kc_finish, dim3(blocks((int64_t)np)), dim3(256), 0, st, (const TwSite *)A.sites, (const long long *)A.p_xcnt,
                       (const long long *)A.p_ycnt, (int64_t)np, A.out9, A.bound9, A.status, A.logs, A.log_bound);
    hipLaunchKernelGGL(kn_combine, dim3(blocks(NS)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_rank_small = (int64_t)h.n_small; S.n_rank_large = (int64_t)h.n_large;
    if (h.decline != CMP_NO_DECLINE) return cur_decline_head(c, status, h);
    unsigned bh_flags = 0;
    if (A.fdr) {
        const auto t0 = std::chrono::steady_clock::now();
        FdrBuf B;
        if (int rc = fdr_alloc(pool, NS, &B)) return rc;
        for (int col = 0; col < 4; ++col) {
            unsigned flags = 0;
            if (int rc = fdr_column(st, B, A.comb + col, A.comb_bound + col, 4, NS, nullptr, A.nlq + col, 4, &flags)) return rc;
            bh_flags |= flags;
            ++S.n_fdr_columns;
        }
        S.ms_fdr = ms_since(t0);
        if (bh_flags & BH_RANGE) return cur_decline(c, status, MC_CMP_DECLINE_FAR_TAIL, 0, -1);
        if (bh_flags & BH_TIE) return cur_decline(c, status, MC_CMP_DECLINE_TIE, 0, -1);
    }
    hipLaunchKernelGGL(kn_size, dim3(blocks(NS)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.row_len, NS, A.row_off, &d_head->out_bytes);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.bed_len, NS, A.bed_off, &d_head->bed_bytes);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.decline != CMP_NO_DECLINE) return cur_decline_head(c, status, h);
    const size_t ob = (size_t)h.out_bytes, bb = (size_t)h.bed_bytes;
    if (!cmp_fits(ob + bb + ((size_t)1 << 20))) return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    if (pool.get(&A.out, ob + 1) || pool.get(&A.bed, bb + 1)) return -10;
    hipLaunchKernelGGL(kn_write, dim3(blocks(NS)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = cur_fetch(c, c->cur_out, c->cur_out_cap, A.out, ob, &res->out, &res->n_out)) return rc;
    if (int rc = cur_fetch(c, c->cur_bed, c->cur_bed_cap, A.bed, bb, &res->bed, &res->n_bed)) return rc;
    S.ms_d2h = ms_since(t_d2h);
    S.n_out_bytes = (int64_t)ob; S.n_bed_bytes = (int64_t)bb; S.n_sig = (int64_t)h.n_sig;
    res->n_sites = NS; res->n_sig = (int64_t)h.n_sig;
    return 0;
}

int cur_call(mc_ctx *c, const mc_text_source &s1, const mc_text_source &s2, const mc_cur_options &opt, mc_cur_result *res, int32_t *status) {
    HIP_TRY(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    c->cur_stats = mc_cur_stats();
    c->cur_stats.decline_line = -1;
    c->cur_stats.n_bytes1 = s1.n_bytes; c->cur_stats.n_bytes2 = s2.n_bytes; c->cur_stats.n_columns = opt.n_columns;
    *res = mc_cur_result();
    *status = 0;
    if (!cmp_fits((size_t)(s1.n_bytes + s2.n_bytes) + 4096)) return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
    Pool pool("current comparison");
    TextFeed feed(c, (size_t)32 << 20);
    char *d_text = nullptr, last1 = '\n';
    if (pool.get(&d_text, (size_t)(s1.n_bytes + s2.n_bytes) + 1 + 64)) return -10;
    if (int rc = feed.send(s1, d_text, &last1)) return rc;
    int64_t off2 = s1.n_bytes;
    if (s1.n_bytes > 0 && last1 != '\n') {                             // the native text's last line ends where the control's first begins
        HIP_TRY(hipMemsetAsync(d_text + off2, '\n', 1, c->up_stream));
        ++off2;
    }
    if (int rc = feed.send(s2, d_text + off2)) return rc;
    if (int rc = feed.pad_and_wait(d_text + off2 + s2.n_bytes)) return rc;
    feed.times(c->cur_stats, t0);
    const auto t_kernels = std::chrono::steady_clock::now();
    const int rc = cur_run(c, pool, d_text, off2 + s2.n_bytes, off2, opt, res, status);
    (void)hipStreamSynchronize(c->stream);                             // (an early return: nothing of the pool is in use when it goes)
    c->cur_stats.ms_kernels = ms_since(t_kernels) - c->cur_stats.ms_d2h;
    if (rc != 0 || *status != 0) *res = mc_cur_result();
    c->cur_stats.ms_total = ms_since(t0);
    return rc;
}
