// mc_sitestats.inc -- the two statistics columns of make_bed -p on the device (included by mc_bedsum.hip, inside its unnamed
// namespace, behind the bucket kernels): make_bed.py:115-127 with the arithmetic and the error bounds of mc_tstat.h.
//   kq_counts          a lane per counted row: its number of values (kb_parse counted the commas) against the first counted row's
//   kq_features        a lane per NUMBER (row of a bucket x value): the token by mc_decimal.h into the fp64 matrix X, one row per
//                      bucket place -- an entry's rows lie together, in ascending row order (kb_place, kb_sort_*)
//   kq_moments_small   entries of up to BS_SMALL rows: a lane per (entry, column)
//   kq_moments_large   deeper ones (the list kb_sort_small made): a wave per (entry, column), lane l the rows l, l + 64, ...;
//                      the 64 partial sums are merged in a fixed tree.  Both: compensated sums (TsSum) of x, then of (x - mean)^2;
//                      the order depends on the row order alone, never on arrival
//   kq_finish          a lane per entry: t and log10 p of every column but the last with their bounds (TsSite), the largest t,
//                      the sum, np.round(., 3), the tie test, the digits (mc_rowtext.h) -- or the decline, named by the entry's first row

__global__ __launch_bounds__(256) void kq_counts(BsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines || !(A.fl[li] & BS_F_COUNTED)) return;
    const int64_t first = (int64_t)A.head->first_counted;
    const uint32_t nv = A.nval[li], ref = A.nval[first];
    if (nv < 2u) line_flag(&A.head->decline, li, MC_BED_DECLINE_FEW_VALUES);
    else if (nv > (uint32_t)MC_BED_MAX_VALUES) line_flag(&A.head->decline, li, MC_BED_DECLINE_MANY_VALUES);
    else if (nv != ref) line_flag(&A.head->decline, li, MC_BED_DECLINE_VALUE_COUNT);
    if (li == first) A.head->nv = (int)nv;
}

__global__ __launch_bounds__(256) void kq_features(BsArgs A, int64_t n_num) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_num) return;
    const int64_t s = idx / A.nv;
    const int j = (int)(idx - s * A.nv);
    const int64_t li = A.bucket[s];
    const TabSpan R = bs_row(A, li);
    const char *t = A.text + A.line_start[li];
    int b = R.t[3] + 1, k = 0;                                         // field 5 = (t3, t4): to the j-th comma
    const int fe = R.t[4];
    for (; k < j && b < fe; ++b) k += t[b] == ',';
    int e = b;
    while (e < fe && t[e] != ',') ++e;
    double v = 0.0;
    if (k != j || !dc_parse(t + b, e - b, &v)) line_flag(&A.head->decline, li, MC_BED_DECLINE_VALUE);
    A.X[idx] = v;
}

struct BqMoments { double mean, ss, sum_abs; };

__device__ __forceinline__ void bq_store_moments(const BsArgs &A, int64_t at, const BqMoments &M) {
    A.mom[3 * at] = M.mean; A.mom[3 * at + 1] = M.ss; A.mom[3 * at + 2] = M.sum_abs;
}

__global__ __launch_bounds__(256) void kq_moments_small(BsArgs A, int64_t n_sel) {
    const int ncol = A.nv - 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_sel * ncol) return;
    const int64_t k = idx / ncol;
    const int j = (int)(idx - k * ncol);
    const uint32_t li = A.sel_line[k];
    const uint32_t depth = A.ent_depth[A.row_ent[li]];
    if (depth < 2u || depth > (uint32_t)BS_SMALL) return;
    const double *x = A.X + (size_t)A.ent_boff[li] * A.nv + j;
    TsSum sum, sq;
    BqMoments M;
    M.sum_abs = 0.0;
    for (uint32_t i = 0; i < depth; ++i) { const double v = x[(size_t)i * A.nv]; sum.add(v); M.sum_abs += fabs(v); }
    M.mean = sum.value() / (double)depth;
    for (uint32_t i = 0; i < depth; ++i) { const double d = x[(size_t)i * A.nv] - M.mean; sq.add(d * d); }
    M.ss = sq.value();
    bq_store_moments(A, idx, M);
}

// the 64 lanes' sums into one, the same tree whatever the data: lane l takes lane l ^ o for o = 32 .. 1 (every lane ends with the total)
__device__ __forceinline__ TsSum bq_wave_sum(TsSum v) {
    for (int o = 32; o > 0; o >>= 1) {
        TsSum w;
        w.s = __shfl_xor(v.s, o); w.c = __shfl_xor(v.c, o);
        const int lane = threadIdx.x & 63;
        TsSum lo = (lane & o) ? w : v, hi = (lane & o) ? v : w;        // both partners add in the same order: the same bits
        lo.merge(hi);
        v = lo;
    }
    return v;
}

__global__ __launch_bounds__(256) void kq_moments_large(BsArgs A) {
    const int ncol = A.nv - 1, lane = threadIdx.x & 63;
    const int64_t n_work = (int64_t)A.head->n_large * ncol;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_work; w += (int64_t)gridDim.x * 4) {
        const int64_t k = A.large[w / ncol];
        const int j = (int)(w % ncol);
        const uint32_t li = A.sel_line[k];
        const uint32_t depth = A.ent_depth[A.row_ent[li]];
        const double *x = A.X + (size_t)A.ent_boff[li] * A.nv + j;
        TsSum sum, sq, ab;
        for (uint32_t i = lane; i < depth; i += 64) { const double v = x[(size_t)i * A.nv]; sum.add(v); ab.add(fabs(v)); }
        sum = bq_wave_sum(sum); ab = bq_wave_sum(ab);
        BqMoments M;
        M.mean = sum.value() / (double)depth;
        for (uint32_t i = lane; i < depth; i += 64) { const double d = x[(size_t)i * A.nv] - M.mean; sq.add(d * d); }
        sq = bq_wave_sum(sq);
        M.ss = sq.value();
        M.sum_abs = ab.value();
        if (lane == 0) bq_store_moments(A, k * ncol + j, M);
    }
}

__device__ __forceinline__ void bq_store_num(const BsArgs &A, size_t at, const RtNum &n, bool is_nan) {
    uint64_t lo;
    uint32_t meta;
    rt_num_pack(n, &lo, &meta);
    A.st_lo[at] = lo;
    A.st_meta[at] = meta | (is_nan ? BS_META_NAN : 0u);
}

__global__ __launch_bounds__(256) void kq_finish(BsArgs A, int64_t n_sel) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const int ncol = A.nv - 1;
    const uint32_t li = A.sel_line[k];
    const uint32_t rep = A.row_ent[li];
    const uint32_t depth = A.ent_depth[rep];
    if (depth < 2u) {                                                  // the host's nan: no variance with one row
        bq_store_num(A, 2 * (size_t)rep, RtNum(), true);
        bq_store_num(A, 2 * (size_t)rep + 1, RtNum(), true);
        return;
    }
    TsSite site;
    for (int j = 0; j < ncol; ++j) {
        const double *m = A.mom + 3 * (k * ncol + j);
        site.column((double)depth, m[0], m[1], m[2]);
    }
    double v_t, v_sum;
    const int flags = site.finish(&v_t, &v_sum);
    const RtNum n_t = rt_num_of(v_t), n_sum = rt_num_of(v_sum);
    int reason = 0;
    if (flags & TS_DEEP) reason = MC_BED_DECLINE_DEPTH;
    else if (flags & TS_ZERO_VAR) reason = MC_BED_DECLINE_ZERO_VARIANCE;
    else if (flags & TS_FAR_TAIL) reason = MC_BED_DECLINE_FAR_TAIL;
    else if (!n_t.ok || !n_sum.ok) reason = MC_BED_DECLINE_PRINT_RANGE;      // (before the tie: from 1e9 up a double has no thousandths left)
    else if (flags & (TS_TIE | TS_NO_CONVERGENCE | TS_BAD_N)) reason = MC_BED_DECLINE_ROUNDING_TIE;      // (no value to vouch for)
    if (reason) { line_flag(&A.head->decline, li, reason); return; }
    bq_store_num(A, 2 * (size_t)rep, n_t, false);
    bq_store_num(A, 2 * (size_t)rep + 1, n_sum, false);
}
