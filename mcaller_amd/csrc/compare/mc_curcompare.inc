// mc_curcompare.inc -- a native sample against an unmodified control, site by site and WITHOUT a model: the rows of
// compare_currents.compare_currents made on the GPU from the texts of two .diffs files (C ABI: mc_currents_compare,
// mc_currents_compare_last_stats, mc_currents_compare_release; Python: Device.currents_compare,
// compare_currents.compare_currents_device).  Part of the mc_bedcompare.hip unit, included behind mc_sitegroup.inc: the grouping of the
// two files' lines by site is that file's (SgArgs, kn_parse .. kn_place, the host phases of SgRun), the statistics on the grouped rows are
// this one's.  It calls kc_rank_small, both kc_rank_large instances, kc_finish and kc_fdr_* (fdr_column) as they are.
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
// none); a line is native when it starts before the control's text.  The steps (S kept sites, c columns, R rows of kept sites):
//   mc_sitegroup.inc with two files   the line starts, kn_parse, kn_group, kn_select<2>, kn_sites<2>, kn_claim, kn_place: the kept
//                sites in the order of their first native rows, every site's native and control rows in ascending line order; more
//                than TW_MAX_N rows at a site decline it (pooled_cap)
//   kn_pseudo    (site, column) = one pseudo-site of RankArgs: offsets and counts into column-major arrays
//   kn_values    a lane per NUMBER: cu_value -> x and y, (site, column) one contiguous run each
//   kc_rank_small / kc_rank_large x 2 / kc_finish   over the S c pseudo-sites, unchanged
//   kn_combine   a lane per site: every column's status, the t_j, mc_curcombine.h per test -> L, its bound, the printed nlp
//   kc_fdr_*     (--fdr) fdr_column once per test over the S combined L
//   kn_size / kp_scan x 2 / kn_write   (sg_outputs) per site the row's and the bed line's length (the --sig_bed decision on the
//                PRINTED value), their places, their bytes (mc_rowtext.h); two outputs
// No floating-point atomic anywhere.
// Resources (tools/kres.py, gfx950; none spills or uses scratch, none uses static LDS, every one runs at 8 waves a SIMD; the grouping
// kernels' figures are in mc_sitegroup.inc's header, the kc_* figures of mc_bedcompare.hip's header stand as they were):
//   kn_values   42 VGPRs    kn_size  54    kn_write  64 (the digit generation of mc_rowtext.h)    kn_combine  30    kn_pseudo  18
// Measured (MI355X, at the commit that added the pipeline, when the grouping kernels stood in this file; tools/currents_probe.py,
// profiles/currents_probe.json and profiles/currents_kernel_stats.csv; synthetic `-m A`-like
// pairs of depth 15 .. 60 with six columns, --fdr --sig_bed, file to file, medians of 3, files in the page cache):
//   2000 sites / 12.5 MB    15.9 s -> 0.0047 s (x3400 against the host statement on the same box, 1.32 ms a site and column; the
//                           device's rows and bed equal the host's); kernels 2.0 ms, of which the four q-value columns 0.77 ms
//   20000 sites / 127 MB    0.0183 s on the device (kernels 6.8 ms, the files' way from the page cache 5.8 ms); the host was not timed
//   a run of 2000 sites, by kernel: kn_parse 0.138 ms, kc_rank_large<512> 0.123, kc_finish 0.105, kn_write 0.073, kc_rank_small 0.060,
//   kn_group 0.054, kn_values 0.052, kn_size 0.051, kn_place 0.030, kn_combine 0.015, kn_claim 0.015, kn_pseudo / kn_select / kn_sites
//   0.005 each: the eleven kn_* are 0.44 ms of 1.63 ms, the q-values' sorts (32 kc_fdr_place and kc_fdr_count) and the 38 single-
//   workgroup kp_scan take as much again.  Not measured: other depths and column counts, files that are not in the page cache.
#include "../mc_curcombine.h"

struct CurHead {                             // device-side result block (copied to the host as it is): grouping's, then the comparison's own
    SgHead g;
    long long out_bytes, bed_bytes;          // totals of the scans
    unsigned long long n_small, n_large;     // pseudo-sites each rank kernel took
    unsigned long long n_sig;
};

struct CurArgs {
    SgArgs g;                                // the lines, keys, sites and rows of the two files (mc_sitegroup.inc)
    SgOut o;
    CurHead *head;
    int fdr, by;                             // by: 0 .. 3, -1: no bed
    double log10c, threshold;
    // per pseudo-site (site, column)
    long long *p_xoff, *p_xcnt, *p_yoff, *p_ycnt;
    double *vals;                            // x[0, c n_rx) then y[0, c n_ry)
    TwSite *sites;
    double *out9, *bound9, *logs, *log_bound;
    int32_t *status;
    // per site: the four combined L, their bounds, the printed nlp, the printed nlq
    double *comb, *comb_bound, *nlp, *nlq;
};

__global__ __launch_bounds__(256) void kn_pseudo(CurArgs A) {
    const SgArgs &G = A.g;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= G.S * G.c) return;
    const int64_t s = p / G.c, j = p % G.c;
    A.p_xoff[p] = G.c * G.off1[s] + j * G.cnt1[s]; A.p_xcnt[p] = G.cnt1[s];
    A.p_yoff[p] = G.c * G.off2r[s] + j * G.cnt2[s]; A.p_ycnt[p] = G.cnt2[s];
}

// a lane per NUMBER: value j of the row at place r -> the column-major arrays
__global__ __launch_bounds__(256) void kn_values(CurArgs A) {
    const SgArgs &G = A.g;
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (G.n_rx + G.n_ry) * G.c) return;
    const int64_t r = v / G.c;
    const int j = (int)(v % G.c);
    const int64_t li = G.rows[r];
    if (li >= G.n_lines) return;
    const CuRow R = cu_row(G, li);
    if (R.s < 0) return;
    const long long place = r - R.off;
    if (place < 0 || place >= R.n) return;
    const double d = cu_value(G, li, j);
    const long long base = R.control ? G.c * G.n_rx + G.c * G.off2r[R.s] : G.c * G.off1[R.s];
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
    if (s >= A.g.S) return;
    const int c = A.g.c;
    const double nan = __builtin_nan("");
    for (int i = 0; i < 4; ++i) { A.comb[s * 4 + i] = nan; A.comb_bound[s * 4 + i] = 0.0; A.nlp[s * 4 + i] = nan; }
    int st = 0;
    for (int j = 0; j < c; ++j) st |= A.status[s * c + j];
    if (st) { line_flag(&A.g.head->decline, A.g.head_line[s], cu_tw_reason(st)); return; }
    for (int i = 0; i < 4; ++i) {
        CcMin M;
        for (int j = 0; j < c; ++j) M.column(A.logs[(s * c + j) * CMP_LOGS + i], A.log_bound[(s * c + j) * CMP_LOGS + i]);
        double L, b, rounded;
        const int cc = M.finish(A.log10c, &L, &b, &rounded);
        if (cc) {
            const int reason = (cc & CC_NAN) ? MC_CMP_DECLINE_NAN : (cc & CC_RANGE) ? MC_CMP_DECLINE_FAR_TAIL
                             : (cc & CC_UNPRINTABLE) ? MC_CMP_DECLINE_PRINT : MC_CMP_DECLINE_TIE;
            line_flag(&A.g.head->decline, A.g.head_line[s], reason);
            continue;
        }
        A.comb[s * 4 + i] = L; A.comb_bound[s * 4 + i] = b; A.nlp[s * 4 + i] = rounded;
    }
}

// the printed value --sig_bed goes by, and the bed line prints
__device__ __forceinline__ double bed_value(const CurArgs &A, int64_t s) { return (A.fdr ? A.nlq : A.nlp)[s * 4 + A.by]; }

// chrom pos pos+1 context strand n_native n_control t_1 .. t_c, the four nlp, (--fdr) the four nlq
template <class Sink>
__device__ __forceinline__ void put_row(const CurArgs &A, int64_t s, Sink &o) {
    const long long li = A.g.head_line[s];
    const TabSpan L = cu_line(A.g, li);
    const char *p = A.g.text + A.g.line_start[li];
    const int c = A.g.c;
    cu_put_prefix(p, L, o);
    cu_put_strand_n(p, L, A.g.cnt1[s], '\t', o);
    rt_put_uint(o, (uint32_t)A.g.cnt2[s]); o.put('\t');
    for (int j = 0; j < c; ++j) { rt_put_num(o, rt_num_of(A.out9[(s * c + j) * TW_N_OUT + 3])); o.put('\t'); }
    for (int i = 0; i < 4; ++i) { rt_put_num(o, rt_num_of(A.nlp[s * 4 + i])); o.put(i < 3 || A.fdr ? '\t' : '\n'); }
    if (A.fdr)
        for (int i = 0; i < 4; ++i) { rt_put_num(o, rt_num_of(A.nlq[s * 4 + i])); o.put(i < 3 ? '\t' : '\n'); }
}

__global__ __launch_bounds__(256) void kn_size(CurArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool sig = false;
    if (s < A.g.S) {
        A.o.row_len[s] = 0; A.o.bed_len[s] = 0;
        bool ok = true;
        for (int i = 0; i < 4; ++i) {                                  // (a NaN: the site's line has declined the file with its own reason)
            const double v = A.nlp[s * 4 + i], q = A.fdr ? A.nlq[s * 4 + i] : 0.0;
            if (v != v || q != q) { ok = false; break; }
            if (!rt_num_of(v).ok || !rt_num_of(q).ok) { line_flag(&A.g.head->decline, A.g.head_line[s], MC_CMP_DECLINE_PRINT); ok = false; break; }
        }
        if (ok) {
            RtCount count;
            put_row(A, s, count);
            A.o.row_len[s] = count.n;
            if (A.by >= 0 && bed_value(A, s) >= A.threshold) {
                RtCount bed;
                cu_put_bed(A.g, s, bed_value(A, s), bed);
                A.o.bed_len[s] = bed.n;
                sig = true;
            }
        }
    }
    const unsigned long long bal = __ballot(sig);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_sig, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(256) void kn_write(CurArgs A) { sg_write_site(A); }

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
    static const char *const nouns[2] = {"native", "control"};
    return decline_in_file(c->currents.stats, status, "current comparison", cur_reason_text(reason), nouns, reason, file, line);
}

// The texts are on the device (d_text[0, n): the native text, a newline if it lacked its last, the control's from off2 on; padded)
int cur_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, int64_t off2, const mc_cur_options &opt, mc_cur_result *res, int32_t *status) {
    mc_cur_stats &S = c->currents.stats;
    hipStream_t st = c->stream;
    if (n == 0) return 0;
    CurHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    CurArgs A = {};
    SgArgs &G = A.g;
    G.text = d_text; G.n_bytes = n; G.files = 2; G.off2 = off2; G.depth = opt.depth; G.c = opt.n_columns; G.pooled_cap = TW_MAX_N;
    A.head = d_head; A.fdr = opt.fdr != 0; A.by = opt.by; A.log10c = opt.log10c; A.threshold = opt.threshold;
    SgRun R{pool, st, G, h.g, [&](int reason, long long line) {           // a line of the texts -> the file it is of and its line there
                const bool first = line < h.g.n_lines1;
                return line < 0 ? cur_decline(c, status, reason, 0, -1) : cur_decline(c, status, reason, first ? 1 : 2, first ? line : line - h.g.n_lines1);
            }};
    const int rc_keys = R.keys(&d_head->g, sizeof *d_head);
    S.n_lines1 = h.g.n_lines1; S.n_lines2 = R.n_lines2; S.table_slots = R.n_slots;
    S.n_keys = (int64_t)h.g.n_keys; S.longest_probe = h.g.longest_probe; S.deepest_site = h.g.deepest; S.n_sites = G.S;
    if (rc_keys) return std::min(rc_keys, 0);
    const int64_t NS = G.S;
    const size_t ns = (size_t)NS, np = ns * (size_t)G.c;
    // per site beside grouping's: the four columns of SgOut, the 16 doubles of comb .. nlq; per pseudo-site; the q-values' buffers
    if (int rc = R.sites(ns * (4 * 8 + 16 * 8) + np * (4 * 8 + sizeof(TwSite) + 2 * 8 * TW_N_OUT + 2 * 8 * CMP_LOGS + 4) + (A.fdr ? fdr_bytes(NS) : 0)))
        return std::min(rc, 0);
    if (pool.get(&A.o.row_len, ns) || pool.get(&A.o.row_off, ns) || pool.get(&A.o.bed_len, ns) || pool.get(&A.o.bed_off, ns) ||
        pool.get(&A.p_xoff, np) || pool.get(&A.p_xcnt, np) || pool.get(&A.p_yoff, np) || pool.get(&A.p_ycnt, np) || pool.get(&A.sites, np) ||
        pool.get(&A.out9, np * TW_N_OUT) || pool.get(&A.bound9, np * TW_N_OUT) || pool.get(&A.logs, np * CMP_LOGS) ||
        pool.get(&A.log_bound, np * CMP_LOGS) || pool.get(&A.status, np) || pool.get(&A.comb, 4 * ns) || pool.get(&A.comb_bound, 4 * ns) ||
        pool.get(&A.nlp, 4 * ns) || pool.get(&A.nlq, 4 * ns))
        return -10;
    HIP_TRY(hipMemsetAsync(A.sites, 0, np * sizeof(TwSite), st));
    HIP_TRY(hipMemsetAsync(A.nlq, 0, 4 * ns * 8, st));
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const size_t nv = (size_t)(h.g.n_rx + h.g.n_ry) * (size_t)G.c;
    S.n_values = (int64_t)nv;
    if (int rc = R.place(nv * 8)) return std::min(rc, 0);
    if (pool.get(&A.vals, nv + 1)) return -10;
    HIP_TRY(hipMemsetAsync(A.vals, 0, (nv + 1) * 8, st));
    hipLaunchKernelGGL(kn_pseudo, dim3(blocks((int64_t)np)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kn_values, dim3(blocks((int64_t)nv)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    RankArgs K = {A.vals, A.vals + (size_t)G.c * (size_t)G.n_rx, A.p_xoff, A.p_xcnt, A.p_yoff, A.p_ycnt, (int64_t)np, A.sites, &d_head->n_small,
                  &d_head->n_large};
    if (int rc = launch_ranks(st, K)) return rc;
    hipLaunchKernelGGL(kc_finish, dim3(blocks((int64_t)np)), dim3(256), 0, st, (const TwSite *)A.sites, (const long long *)A.p_xcnt,
                       (const long long *)A.p_ycnt, (int64_t)np, A.out9, A.bound9, A.status, A.logs, A.log_bound);
    hipLaunchKernelGGL(kn_combine, dim3(blocks(NS)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_rank_small = (int64_t)h.n_small; S.n_rank_large = (int64_t)h.n_large;
    if (h.g.decline != CMP_NO_DECLINE) { R.stop_head(); return 0; }
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
    if (int rc = sg_outputs(c, R, A, d_head, h, kn_size, kn_write, c->currents.out, c->currents.bed, S, res)) return std::min(rc, 0);
    S.n_sig = (int64_t)h.n_sig;
    res->n_sites = NS; res->n_sig = (int64_t)h.n_sig;
    return 0;
}

int cur_call(mc_ctx *c, const mc_text_source &s1, const mc_text_source &s2, const mc_cur_options &opt, mc_cur_result *res, int32_t *status) {
    mc_cur_stats &S = c->currents.stats;
    return pipeline_call(c, S, status, "current comparison", (size_t)32 << 20, [&] { *res = mc_cur_result(); }, [&](Call &K) -> int {
        S.n_bytes1 = s1.n_bytes; S.n_bytes2 = s2.n_bytes; S.n_columns = opt.n_columns;
        if (!cmp_fits((size_t)(s1.n_bytes + s2.n_bytes) + 4096)) return cur_decline(c, status, MC_CMP_DECLINE_MEMORY, 0, -1);
        char *d_text = nullptr;
        int64_t off2 = 0;
        if (K.pool.get(&d_text, (size_t)(s1.n_bytes + s2.n_bytes) + 1 + 64)) return -10;
        if (int rc = K.feed.put_pair(s1, &s2, d_text, &off2)) return rc;
        K.feed.times(S, K.t0);
        const auto t_kernels = std::chrono::steady_clock::now();
        const int rc = cur_run(c, K.pool, d_text, off2 + s2.n_bytes, off2, opt, res, status);
        S.ms_kernels = ms_since(t_kernels) - S.ms_d2h;        // a declined call too: what ran until it declined
        return rc;
    });
}
