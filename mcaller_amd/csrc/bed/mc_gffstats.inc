// mc_gffstats.inc -- the three attributes make_bed --gff --vo adds to an entry (included by mc_bedsum.hip, inside its unnamed
// namespace, behind the bucket kernels): make_bed.py:146-149 with the arithmetic of mc_npsum.h -- NumPy's own order of additions,
// so the values are the host's bit for bit and no bound is needed.
//   kg_probs           a lane per bucket place (a counted row): the stripped probability text of a row of a SELECTED entry by
//                      mc_decimal.h into fp64 (the host calls float() for written entries only) -- an entry's rows lie together, in
//                      ascending row order (kb_place, kb_sort_*)
//   kg_moments_small   a lane per selected entry of up to NS_BLOCK rows, one leaf of the tree: 0.0 + pw(p), the mean, 0.0 + pw of the
//                      rounded squares; a deeper entry goes onto a list
//   kg_moments_large   a workgroup per deeper entry: chunk by chunk of NS_CHUNK rows in order, thread k is node k of the chunk's tree
//                      (ns_node): a leaf sums its up to NS_BLOCK elements, then the levels are combined from the deepest up, left
//                      + right as the recursion adds them; thread 0 joins the chunks.  Two sweeps: the sum, then the squares
//   kg_finish          a lane per selected entry: fracLow, fracUp (their digits by mc_rowtext.h) and 100 * mean -- or the decline,
//                      named by the entry's first row
// No floating-point atomics; nothing depends on the order of arrival (the list of deep entries is in arrival order, their values are not).

__global__ __launch_bounds__(256) void kg_probs(BsArgs A, int64_t n_counted) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_counted) return;
    const int64_t li = A.bucket[s];
    double v = 0.0;
    if (bs_selected(A, A.row_ent[li])) {
        const uint32_t ps = A.pspan[li];
        if (!dc_parse(A.text + A.line_start[li] + (ps >> 16), (int)(ps & 0xffffu), &v)) line_flag(&A.head->decline, li, MC_BED_DECLINE_PROBABILITY);
    }
    A.X[s] = v;
}

__global__ __launch_bounds__(256) void kg_moments_small(BsArgs A, int64_t n_sel) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const uint32_t li = A.sel_line[k];
    const uint32_t depth = A.ent_depth[A.row_ent[li]];
    if (depth > (uint32_t)NS_BLOCK) { A.g_large[atomicAdd(&A.head->g_n_large, 1u)] = (uint32_t)k; return; }
    const double *p = A.X + A.ent_boff[li];
    const double sum = 0.0 + ns_leaf(NsPlain{p}, 0, (int)depth);
    const double mean = sum / (double)depth;
    A.mom[2 * k] = mean;
    A.mom[2 * k + 1] = 0.0 + ns_leaf(NsSquare{p, mean}, 0, (int)depth);
}

// A workgroup of NS_NODES threads, every one of them here: the mean and the sum of the squares of x[0, depth) -> thread 0's *mean and *ss
__device__ __forceinline__ void gs_block_moments(const double *__restrict__ x, int64_t depth, double *s_val, int *s_len, double *s_mean,
                                                 double *mean_out, double *ss_out) {
    const int k = threadIdx.x;                                         // the node of the chunk's tree (0: none)
    for (int sweep = 0; sweep < 2; ++sweep) {
        const double mean = sweep ? *s_mean : 0.0;
        double r = 0.0;                                                // (thread 0's: the chunks joined in order)
        for (int64_t c0 = 0; c0 < depth; c0 += NS_CHUNK) {
            const int m = (int)(depth - c0 < NS_CHUNK ? depth - c0 : NS_CHUNK);
            int a = 0, n = 0;
            const bool have = k >= 1 && ns_node(m, k, &a, &n);
            s_len[k] = have ? n : 0;
            if (have && n <= NS_BLOCK) s_val[k] = sweep ? ns_leaf(NsSquare{x, mean}, c0 + a, n) : ns_leaf(NsPlain{x}, c0 + a, n);
            __syncthreads();
            for (int level = 6; level >= 0; --level) {                 // (level 7, nodes 128 .. 255, holds leaves only: mc_npsum.h)
                if (k >= (1 << level) && k < (2 << level) && k < NS_NODES / 2 && s_len[k] > NS_BLOCK) s_val[k] = s_val[2 * k] + s_val[2 * k + 1];
                __syncthreads();
            }
            if (k == 0) r = r + s_val[1];
            __syncthreads();
        }
        if (k == 0) {
            if (sweep == 0) { *s_mean = r / (double)depth; *mean_out = *s_mean; }
            else *ss_out = r;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NS_NODES) void kg_moments_large(BsArgs A) {
    __shared__ double s_val[NS_NODES];
    __shared__ int s_len[NS_NODES];
    __shared__ double s_mean;
    const unsigned n_large = A.head->g_n_large;
    for (unsigned q = blockIdx.x; q < n_large; q += gridDim.x) {
        const int64_t e = A.g_large[q];
        const uint32_t li = A.sel_line[e];
        double mean = 0.0, ss = 0.0;
        gs_block_moments(A.X + A.ent_boff[li], (int64_t)A.ent_depth[A.row_ent[li]], s_val, s_len, &s_mean, &mean, &ss);
        if (threadIdx.x == 0) { A.mom[2 * e] = mean; A.mom[2 * e + 1] = ss; }
    }
}

__global__ __launch_bounds__(256) void kg_finish(BsArgs A, int64_t n_sel) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const uint32_t li = A.sel_line[k];
    const uint32_t rep = A.row_ent[li];
    const uint32_t depth = A.ent_depth[rep];
    double out3[3];
    const int st = ns_finish(A.mom[2 * k], A.mom[2 * k + 1], (int64_t)depth, (double)A.ent_meth[rep] / (double)depth, out3);
    if (st & NS_QV_RANGE) { line_flag(&A.head->decline, li, MC_BED_DECLINE_QV_RANGE); return; }
    if (st & NS_PRINT_RANGE) { line_flag(&A.head->decline, li, MC_BED_DECLINE_STAT_RANGE); return; }
    for (int q = 0; q < 2; ++q) {
        const bool is_nan = !(out3[q] == out3[q]);
        bq_store_num(A, 2 * (size_t)rep + q, is_nan ? RtNum() : rt_num_of(out3[q]), is_nan);
    }
    A.g_qv[rep] = out3[2];
}

// the probes of mc_npsum.h's device build: a workgroup per array, by the two kernels' own steps (up to NS_BLOCK elements: the leaf)
__global__ __launch_bounds__(NS_NODES) void k_ns_probe(const double *__restrict__ p, const long long *__restrict__ off, const double *__restrict__ frac,
                                                       int64_t count, double *__restrict__ out6, int32_t *__restrict__ status) {
    __shared__ double s_val[NS_NODES];
    __shared__ int s_len[NS_NODES];
    __shared__ double s_mean;
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        const double *x = p + off[q];
        const int64_t depth = off[q + 1] - off[q];
        double mean = 0.0, ss = 0.0;
        if (depth > NS_BLOCK) gs_block_moments(x, depth, s_val, s_len, &s_mean, &mean, &ss);
        else if (threadIdx.x == 0) {
            mean = (0.0 + ns_leaf(NsPlain{x}, 0, (int)depth)) / (double)depth;
            ss = 0.0 + ns_leaf(NsSquare{x, mean}, 0, (int)depth);
        }
        if (threadIdx.x == 0) {
            double out3[3];
            const double var = ss / (double)(depth - 1);
            status[q] = ns_finish(mean, ss, depth, frac[q], out3);
            out6[6 * q] = out3[0]; out6[6 * q + 1] = out3[1]; out6[6 * q + 2] = out3[2];
            out6[6 * q + 3] = mean; out6[6 * q + 4] = var; out6[6 * q + 5] = ns_se(var, (double)depth);
        }
    }
}

__global__ __launch_bounds__(256) void k_ns_se_probe(const double *__restrict__ var, const double *__restrict__ n, int64_t count, double *__restrict__ se) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) se[i] = ns_se(var[i], n[i]);
}
