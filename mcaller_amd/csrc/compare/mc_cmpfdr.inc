// mc_cmpfdr.inc -- the count test and the multiple-testing correction of compare_genomes on the GPU (part of mc_bedcompare.hip; the
// definition: mcaller_amd/compare_genomes.py, fisher_nlp and bh_log10).  C ABI: mc_bed_compare_with's options (the file pipeline:
// cmp_extra_columns, between kc_finish and kc_size), mc_fisher_exact_device, mc_bh_adjust_device (a batch of tables, one column);
// Python: Device.bed_compare(fisher=, fdr=), Device.fisher_exact, Device.bh_adjust.  The arithmetic is mc_fisher.h's and mc_bh.h's,
// which the host build shares.
//
//   kc_fisher_sites  the file pipeline, a lane per shared site: the two lines' frac fields by mc_decimal.h (shared lines only; a line
//                    bed2 lacks is never read), fe_count, fe_log10p -> the site's fifth log10 p with its bound, the printed
//                    nlp_fisher; a frac that is no count, a far tail, a mass at the selection factor, a rounding tie within the
//                    bound or an unprintable value declines the file by line_flag.  Sites are up to 8192 pooled reads deep and a
//                    lane walks its own: 42 us of the 2.65 ms of kernels at 10^4 sites of depth 15 .. 60
//                    (profiles/compare_fdr_kernel_stats.csv), so a wave per deep site has not been needed
//   kc_fisher        a lane per table (K1, n1, K2, n2): fe_log10p -> log10 p, its derived bound, the status bits.  A lane walks its
//                    table's hi - lo + 1 weights twice, so a wave is as slow as its deepest table
//   kc_fdr_keys      a lane per row: the order-preserving 64-bit key of its L (mc_bh.h; a NaN row gets the highest key and stands
//                    behind the m tested rows), its row number as the 32-bit payload.  Into the head by INTEGER atomics whose
//                    results do not depend on the order of arrival: the OR and the AND of the keys, m, the largest bound (atomicMax
//                    on the bits of a non-negative double, which order as the doubles do), the range flag
//   kc_fdr_count / kp_scan / kc_fdr_place   a stable device-wide LSD radix sort of (key, row), 8 bits a pass: digit counts per
//                    workgroup of FR_CHUNK rows, an exclusive scan digit-major, then the scatter -- chunk by chunk of 256 in order,
//                    a row's place = the digit's base + rows of that digit in earlier waves of the chunk + those before it in its
//                    wave (ballots).  A pass whose byte is the same in every key (OR == AND there) is skipped: log10 p of one
//                    column share their sign and most of their exponent, and a column of equal L sorts in no pass at all
//   kc_fdr_terms     a lane per sorted place j < m: T = L + (log10 m - log10(j + 1)); a workgroup's minimum of its 256 terms
//   kc_fdr_behind    one workgroup: for every block of 256 places the minimum of the blocks BEHIND it, from the end in chunks of 1024
//                    with a carry.  Two levels and no look-back: min is order-free, so no arrival order shows in a value
//   kc_fdr_finish    a lane per sorted place: the minimum from its place to its block's end, the blocks behind, bh_finish with the
//                    column bound -> Q and the printed value AT THE ROW'S OWN PLACE (the scatter back to row order), NaN twice for an
//                    untested row; the tie flag by atomicOr
// No floating-point atomic, and no atomic decides an order or a value.
// The file pipeline adjusts its four or five columns one after the other in one set of buffers (fdr_column; one sort a column: the
// key keeps all 64 bits of the double, so there is no room for a column number in it).
// Resources (tools/kres.py, gfx950; none spills or uses scratch; 8 waves a SIMD each): kc_fisher_sites 56 VGPRs, kc_fisher 52,
// kc_fdr_keys 16, kc_fdr_count 7 (1 KB LDS), kc_fdr_place 28 (6 KB LDS: the digit bases and four waves' counts), kc_fdr_terms 28,
// kc_fdr_behind 22, kc_fdr_finish 18.

constexpr int FR_CHUNK = 2048;               // rows a workgroup counts and places per pass: eight rounds of 256

struct FdrHead {                             // device-side result block (copied to the host as it is)
    unsigned long long k_or, k_and;          // over the keys
    unsigned long long m;                    // tested rows
    unsigned long long bound_bits;           // the largest bound of a tested row, as bits
    unsigned int flags, pad;                 // BH_* status bits
    long long scratch;                       // kp_scan's total
};

__global__ __launch_bounds__(256) void kc_fisher(const long long *__restrict__ K1, const long long *__restrict__ n1, const long long *__restrict__ K2,
                                                 const long long *__restrict__ n2, int64_t count, double *__restrict__ log10p,
                                                 double *__restrict__ bound, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double l, b;
    int st;
    fe_log10p(K1[i], n1[i], K2[i], n2[i], &l, &b, &st);
    log10p[i] = l; bound[i] = b; status[i] = st;
}

__global__ __launch_bounds__(256) void kc_fdr_keys(const double *__restrict__ L, const double *__restrict__ bound, int stride, int64_t n,
                                                   unsigned long long *__restrict__ key, uint32_t *__restrict__ row, FdrHead *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long k_or = 0, k_and = ~0ull, b_bits = 0;
    bool tested = false, range = false;
    if (i < n) {
        const double l = L[i * stride], b = bound[i * stride];
        const unsigned long long k = bh_key(l);
        key[i] = k; row[i] = (uint32_t)i;
        k_or = k_and = k;
        range = !bh_in_range(l, b);
        tested = !range && l == l;
        if (tested) b_bits = (unsigned long long)__double_as_longlong(b + 0.0);      // (-0.0 + 0.0: the bits of +0.0)
    }
    for (int o = 32; o > 0; o >>= 1) {
        k_or |= __shfl_xor(k_or, o); k_and &= __shfl_xor(k_and, o);
        const unsigned long long other = __shfl_xor(b_bits, o);
        b_bits = other > b_bits ? other : b_bits;
    }
    const unsigned long long n_tested = __ballot(tested), any_range = __ballot(range);
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&head->k_or, k_or); atomicAnd(&head->k_and, k_and);
        if (n_tested) { atomicAdd(&head->m, (unsigned long long)__popcll(n_tested)); atomicMax(&head->bound_bits, b_bits); }
        if (any_range) atomicOr(&head->flags, (unsigned int)BH_RANGE);
    }
}

// cnt[digit * workgroups + workgroup]: rows of the workgroup's chunk with that digit
__global__ __launch_bounds__(256) void kc_fdr_count(const unsigned long long *__restrict__ key, int64_t n, int sh, long long *__restrict__ cnt) {
    __shared__ unsigned s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * FR_CHUNK;
    for (int i = threadIdx.x; i < FR_CHUNK; i += 256)
        if (c0 + i < n) atomicAdd(&s_hist[(unsigned)(key[c0 + i] >> sh) & 255u], 1u);
    __syncthreads();
    cnt[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (long long)s_hist[threadIdx.x];
}

__global__ __launch_bounds__(256) void kc_fdr_place(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ row, int64_t n, int sh,
                                                    const long long *__restrict__ cnt_off, unsigned long long *__restrict__ key_dst,
                                                    uint32_t *__restrict__ row_dst) {
    __shared__ long long s_base[256];
    __shared__ unsigned s_wc[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = cnt_off[(size_t)tid * gridDim.x + blockIdx.x];
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * FR_CHUNK;
    for (int s0 = 0; s0 < FR_CHUNK && c0 + s0 < n; s0 += 256) {
        const int64_t j = c0 + s0 + tid;
        const bool valid = j < n;
        const unsigned long long k = valid ? key[j] : 0ull;
        const unsigned d = (unsigned)(k >> sh) & 255u;
        unsigned long long peers = __ballot(valid);             // lanes of the wave with a row of the same digit
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(one);
            peers &= one ? bal : ~bal;
        }
        const unsigned before_me = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        const bool leader = valid && before_me == 0;
        for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
        __syncthreads();
        if (leader) s_wc[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (valid) {
            long long at = s_base[d] + before_me;
            for (int w = 0; w < wave; ++w) at += s_wc[w][d];
            key_dst[at] = k; row_dst[at] = row[j];
        }
        __syncthreads();
        s_base[tid] += (long long)(s_wc[0][tid] + s_wc[1][tid] + s_wc[2][tid] + s_wc[3][tid]);      // (tid is the digit here)
        __syncthreads();
    }
}

// the minimum of v over the places of the workgroup at and behind the thread's own (256 threads); s_w: 4 doubles
__device__ __forceinline__ double fdr_block_min_behind(double v, double *s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_down(v, o);
        if (lane + o < 64) v = fmin(v, u);
    }
    __syncthreads();
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    for (int w = wave + 1; w < 4; ++w) v = fmin(v, s_w[w]);
    return v;
}

__global__ __launch_bounds__(256) void kc_fdr_terms(const unsigned long long *__restrict__ key, int64_t n, const FdrHead *__restrict__ head,
                                                    double *__restrict__ T, double *__restrict__ blk_min) {
    __shared__ double s_w[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, m = (int64_t)head->m;
    double t = INFINITY;
    if (j < m) {
        t = bh_term(bh_unkey(key[j]), log10((double)m), j + 1);
        T[j] = t;
    }
    const double behind = fdr_block_min_behind(t, s_w);
    if (threadIdx.x == 0) blk_min[blockIdx.x] = behind;
}

// after[b] = min of blk_min[b + 1 ..]: one workgroup, from the end
__global__ __launch_bounds__(1024) void kc_fdr_behind(const double *__restrict__ blk_min, int64_t nb, double *__restrict__ after) {
    __shared__ double s_w[16];
    __shared__ double s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = INFINITY;
    __syncthreads();
    for (int64_t base = ((nb - 1) / 1024) * 1024; base >= 0; base -= 1024) {
        const int64_t i = base + tid;
        double v = i < nb ? blk_min[i] : INFINITY;
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_down(v, o);
            if (lane + o < 64) v = fmin(v, u);
        }
        const double next = __shfl_down(v, 1);                  // the places behind this one in its wave
        if (lane == 0) s_w[wave] = v;
        __syncthreads();
        double behind = s_carry;
        if (lane < 63) behind = fmin(behind, next);
        for (int w = wave + 1; w < 16; ++w) behind = fmin(behind, s_w[w]);
        if (i < nb) after[i] = behind;
        __syncthreads();
        if (tid == 0) s_carry = fmin(behind, v);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void kc_fdr_finish(const double *__restrict__ T, const uint32_t *__restrict__ row, const double *__restrict__ after,
                                                     int64_t n, FdrHead *__restrict__ head, double *__restrict__ Q, double *__restrict__ rounded,
                                                     int out_stride) {
    __shared__ double s_w[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, m = (int64_t)head->m;
    const double t = j < m ? T[j] : INFINITY;
    const double t_min = fmin(fdr_block_min_behind(t, s_w), after[blockIdx.x]);
    int st = BH_OK;
    if (j < n) {
        const uint32_t r = row[j];
        if (j < m) {
            double q, v;
            st = bh_finish(t_min, __longlong_as_double((long long)head->bound_bits), &q, &v);
            if (Q) Q[(size_t)r * out_stride] = q;
            rounded[(size_t)r * out_stride] = v;
        } else {
            if (Q) Q[(size_t)r * out_stride] = __builtin_nan("");
            rounded[(size_t)r * out_stride] = __builtin_nan("");
        }
    }
    const unsigned long long ties = __ballot(st != BH_OK);
    if (ties && (threadIdx.x & 63) == 0) atomicOr(&head->flags, (unsigned int)BH_TIE);
}

// what a column of n rows holds on the device while it is adjusted, beside its L, bounds and results: both (key, row) arrays of the
// sort, the terms, the digit counts and their scan, the blocks' minima
struct FdrBuf {
    unsigned long long *key[2];
    uint32_t *row[2];
    double *T, *blk, *after;
    long long *cnt, *off;
    FdrHead *head;
};

size_t fdr_bytes(int64_t n) {
    const size_t wgs = (size_t)((n + FR_CHUNK - 1) / FR_CHUNK), nb = (size_t)((n + 255) / 256);
    return (size_t)n * (2 * 8 + 2 * 4 + 8) + 2 * 256 * wgs * 8 + 2 * nb * 8 + sizeof(FdrHead) + ((size_t)1 << 16);
}

int fdr_alloc(Pool &pool, int64_t n, FdrBuf *B) {
    const size_t N = (size_t)n, wgs = (N + FR_CHUNK - 1) / FR_CHUNK, nb = (N + 255) / 256;
    *B = FdrBuf();
    if (pool.get(&B->key[0], N) || pool.get(&B->key[1], N) || pool.get(&B->row[0], N) || pool.get(&B->row[1], N) || pool.get(&B->T, N) ||
        pool.get(&B->blk, nb) || pool.get(&B->after, nb) || pool.get(&B->cnt, 256 * wgs) || pool.get(&B->off, 256 * wgs) || pool.get(&B->head, 1))
        return -10;
    return 0;
}

// One column on the device: L and bound of row i at [i * stride] -> log10 q (d_Q null: not wanted) and the printed value of row i at
// [i * out_stride]; *flags: the BH_* bits.  BH_RANGE: nothing is written.  The stream is waited for (the head is read twice).
int fdr_column(hipStream_t st, const FdrBuf &B, const double *d_L, const double *d_bound, int stride, int64_t n, double *d_Q, double *d_R,
               int out_stride, unsigned *flags) {
    const size_t N = (size_t)n, wgs = (N + FR_CHUNK - 1) / FR_CHUNK, nb = (N + 255) / 256;
    FdrHead h = {};
    h.k_and = ~0ull;
    HIP_TRY(hipMemcpyAsync(B.head, &h, sizeof h, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kc_fdr_keys, dim3(blocks(n)), dim3(256), 0, st, d_L, d_bound, stride, n, B.key[0], B.row[0], B.head);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, B.head, h)) return rc;
    *flags = h.flags;
    if (h.flags & BH_RANGE) return 0;
    int cur = 0;
    const unsigned long long differ = h.k_or ^ h.k_and;
    for (int sh = 0; sh < 64; sh += 8) {
        if (!((differ >> sh) & 255ull)) continue;               // the byte is the same in every key: the order stands
        hipLaunchKernelGGL(kc_fdr_count, dim3((unsigned)wgs), dim3(256), 0, st, (const unsigned long long *)B.key[cur], n, sh, B.cnt);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)B.cnt, (int64_t)(256 * wgs), B.off, &B.head->scratch);
        hipLaunchKernelGGL(kc_fdr_place, dim3((unsigned)wgs), dim3(256), 0, st, (const unsigned long long *)B.key[cur], (const uint32_t *)B.row[cur], n, sh,
                           (const long long *)B.off, B.key[cur ^ 1], B.row[cur ^ 1]);
        HIP_TRY(hipGetLastError());
        cur ^= 1;
    }
    hipLaunchKernelGGL(kc_fdr_terms, dim3((unsigned)nb), dim3(256), 0, st, (const unsigned long long *)B.key[cur], n, (const FdrHead *)B.head, B.T, B.blk);
    hipLaunchKernelGGL(kc_fdr_behind, dim3(1), dim3(1024), 0, st, (const double *)B.blk, (int64_t)nb, B.after);
    hipLaunchKernelGGL(kc_fdr_finish, dim3((unsigned)nb), dim3(256), 0, st, (const double *)B.T, (const uint32_t *)B.row[cur], (const double *)B.after, n,
                       B.head, d_Q, d_R, out_stride);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, B.head, h)) return rc;
    *flags = h.flags;
    return 0;
}

// L and bound on the host -> Q and rounded on the host, *status the BH_* bits
int fdr_adjust(mc_ctx *c, const double *L, const double *bound, int64_t n, double *Q, double *rounded, int32_t *status) {
    hipStream_t st = c->stream;
    const size_t N = (size_t)n;
    if (!cmp_fits(fdr_bytes(n) + N * 4 * 8)) {
        mc_set_error("mc_bh_adjust_device: %lld rows do not fit into free device memory beside their sort buffers", (long long)n);
        return -10;
    }
    Pool pool("Benjamini-Hochberg adjustment");
    double *d_io = nullptr;                                     // L, bound, Q, rounded
    FdrBuf B;
    if (pool.get(&d_io, 4 * N) || fdr_alloc(pool, n, &B)) return -10;
    unsigned flags = 0;
    int rc = mc_hip_rc(hipMemcpyAsync(d_io, L, N * 8, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(d_io + N, bound, N * 8, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
    if (rc == 0) rc = fdr_column(st, B, d_io, d_io + N, 1, n, d_io + 2 * N, d_io + 3 * N, 1, &flags);
    if (rc == 0 && !(flags & BH_RANGE)) {
        rc = mc_hip_rc(hipMemcpyAsync(Q, d_io + 2 * N, N * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(rounded, d_io + 3 * N, N * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    }
    const int rc_sync = mc_hip_rc(hipStreamSynchronize(st), "hipStreamSynchronize");      // (nothing of the pool is in use when it goes)
    if (rc || rc_sync) return rc ? rc : rc_sync;
    if (flags & BH_RANGE)
        for (size_t i = 0; i < N; ++i) Q[i] = rounded[i] = __builtin_nan("");
    *status = (int32_t)(flags & (BH_TIE | BH_RANGE));
    return 0;
}

// ---- the file pipeline's share (mc_bed_compare_with): behind kc_finish, before kc_size ----

// a lane per site: the two lines' counts from their frac fields (mc_decimal.h, fe_count), fe_log10p -> the site's fifth log10 p and
// its bound, the printed nlp_fisher as the row's first extra column; a line that is no count, or a value that cannot be vouched
// for, declines its file
__global__ __launch_bounds__(256) void kc_fisher_sites(CmpArgs A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.S) return;
    long long K[2] = {0, 0};
    const long long n[2] = {A.cnt1[s], A.cnt2[s]};
    bool sound = true;
    for (int side = 0; side < 2; ++side) {
        const long long li = side ? A.line2[s] : A.line1[s];
        const TabSpan L = cmp_line(A, li);
        double f = 0.0;
        int64_t k = 0;
        if (!dc_parse(A.text + A.line_start[li] + L.t[3] + 1, L.t[4] - L.t[3] - 1, &f) || !fe_count(f, n[side], &k)) {
            line_flag(&A.head->decline, li, MC_CMP_DECLINE_FRAC);
            sound = false;
        }
        K[side] = k;
    }
    double l = __builtin_nan(""), b = 0.0;
    if (sound) {
        int st;
        fe_log10p(K[0], n[0], K[1], n[1], &l, &b, &st);
        double lo = -l - b, hi = -l + b;
        if (!(lo > 0.0)) lo = 0.0;
        if (!(hi > 0.0)) hi = 0.0;
        const int reason = (st & (FE_BAD_ARGS | FE_FAR_TAIL)) ? MC_CMP_DECLINE_FAR_TAIL : (st & FE_SELECT) ? MC_CMP_DECLINE_FISHER_SELECT
                         : ts_tie_between(lo, hi) ? MC_CMP_DECLINE_TIE : !rt_num_of(tw_nlp(l)).ok ? MC_CMP_DECLINE_PRINT : 0;
        if (reason) line_flag(&A.head->decline, A.line1[s], reason);
    }
    A.logs[s * CMP_LOGS + 4] = l; A.log_bound[s * CMP_LOGS + 4] = b;
    A.extra[s * A.n_extra] = tw_nlp(l);
}

// the columns behind nlp_ks of every site, behind kc_finish: nlp_fisher (kc_fisher_sites), then a column of q-values for each of the
// four tests and for Fisher's -- one sort a column, the columns one after the other in the same buffers.  *bh_flags: the BH_* bits
// of all columns
int cmp_extra_columns(mc_ctx *c, Pool &pool, const CmpArgs &A, unsigned *bh_flags) {
    hipStream_t st = c->stream;
    mc_cmp_stats &S = c->cmp.stats;
    HIP_TRY(hipMemsetAsync(A.extra, 0, (size_t)A.S * (size_t)A.n_extra * 8, st));
    if (A.fisher) {
        hipLaunchKernelGGL(kc_fisher_sites, dim3(blocks(A.S)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        S.n_fisher = A.S;
    }
    if (!A.fdr) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    FdrBuf B;
    if (int rc = fdr_alloc(pool, A.S, &B)) return rc;
    for (int col = 0; col < 4 + A.fisher; ++col) {
        unsigned flags = 0;
        if (int rc = fdr_column(st, B, A.logs + col, A.log_bound + col, CMP_LOGS, A.S, nullptr, A.extra + A.fisher + col, A.n_extra, &flags)) return rc;
        *bh_flags |= flags;
        ++S.n_fdr_columns;
    }
    S.ms_fdr = ms_since(t0);
    return 0;
}

int fisher_batch(mc_ctx *c, const int64_t *K1, const int64_t *n1, const int64_t *K2, const int64_t *n2, int64_t count, double *log10_p, double *bound,
                 int32_t *status) {
    hipStream_t st = c->stream;
    Pool pool("Fisher batch");
    const size_t N = (size_t)count;
    long long *d_in = nullptr;
    double *d_out = nullptr;
    int32_t *d_st = nullptr;
    if (pool.get(&d_in, 4 * N) || pool.get(&d_out, 2 * N) || pool.get(&d_st, N)) return -10;
    const int64_t *in[4] = {K1, n1, K2, n2};
    for (int q = 0; q < 4; ++q) HIP_TRY(hipMemcpyAsync(d_in + q * N, in[q], N * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kc_fisher, dim3(blocks(count)), dim3(256), 0, st, (const long long *)d_in, (const long long *)(d_in + N), (const long long *)(d_in + 2 * N),
                       (const long long *)(d_in + 3 * N), count, d_out, d_out + N, d_st);
    int rc = mc_hip_rc(hipGetLastError(), "kc_fisher");
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(log10_p, d_out, N * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(bound, d_out + N, N * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(status, d_st, N * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    const int rc_sync = mc_hip_rc(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc_sync;
}
