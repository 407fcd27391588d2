// libmcaller_hip.so -- the random-forest fit behind `--train -c RF` on the GPU (gfx950 / MI355X).  C ABI: include/mcaller_hip.h.
//
// The reference fits RandomForestClassifier(criterion='entropy', max_depth=10, max_features=4, min_samples_leaf=2,
// min_samples_split=3, n_estimators=50, bootstrap=True) per sub-model, five times for GroupKFold and once more on all rows
// (train_model.py:39-45,:62-65,:92-100).  Every (job, tree) here is one workgroup of k5_forest_fit; no workgroup waits for another.
// The algorithm, its keyed randomness included, is tests/forest_fit_oracle.py, which this follows bit for bit:
//
//   * the host sorts each feature's column of X once per call (float32 values, rows in index order among equal values); a tree
//     keeps, per feature, its in-bag rows in that order (a stable compaction by bootstrap weight): entries (x, row);
//   * the tree grows level by level.  The open nodes of a level own contiguous segments, the same segment in every feature's list,
//     each sorted by that feature;  a lane per (node, visited feature) walks the segment once, the running class weights giving
//     every candidate's score from the G[m] = m ln m table (additions only: the same bits as the CPU);  a lane per node keeps the
//     best (highest score, first visited feature, lowest position);
//   * every feature's list is then stable-partitioned by the side each row went to (one block scan over the list per feature),
//     so the children's segments are sorted again without a sort;
//   * nodes are written in level order with child links; the host renumbers them into scikit-learn's depth-first pre-order.
// A second kernel (k5_forest_val) scores each job's validation rows with its trees in tree order, as k3_forest adds them.
// Work arrays are in global memory, per workgroup; trees are grown in batches that fit MCALLER_FOREST_MEM_MB (default 4096);
// mc_forest_fit_last_stats tells how a call was cut.
// The entry points' allocations, transfers and job checks, FitJob, splitmix64 and wave_sum: mc_fit.h.
#include <cstdlib>
#include <numeric>

#include "mc_fit.h"

mc_forest_fit_stats *mc_internal_forest_stats(mc_ctx *c);      // mc_context.hip: the context's figures of its last forest fit

namespace {

constexpr int BT = 256;                 // threads per tree
constexpr int NWAVE = BT / 64;
constexpr int DMAX = MC_MAX_K + 1;      // features
constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ull, DRAW = 0xD1342543DE82EF95ull, NODEK = 0x632BE59BD9B4E019ull;
constexpr double LN2 = 0.6931471805599453;

struct Ent {                            // a row in a feature's sorted list
    float x;
    int32_t r;
};
struct LNode {                          // an open node of the current level
    int32_t start, end, w0, w1;
    uint64_t h;
};
struct NWork {                          // what a level decides about a node
    double thr;
    int32_t rank, feat, nleft, lbase, nv, leaf;
    int8_t vis[DMAX];                   // visited features in order; +64: constant in the node
};
struct SBest {                          // best split of one (node, visited feature)
    double score;
    int32_t pos, a0, a1, pad;
};
struct FNode {                          // output, level order
    int32_t left, right, feature, n_samples;
    double threshold, v0, v1, impurity, weighted;
};

struct FitArgs {
    const float *Xt;                    // [d][n]
    const int32_t *order;               // [d][n] rows sorted by Xt[f]
    const uint8_t *y;
    const int32_t *tr_idx;
    const FitJob *jobs;
    const double *G;
    int32_t d, n_trees, max_depth, max_features, mss, msl, bootstrap;
    int64_t n;
    int64_t cap_s, cap_lvl, cap_nodes;  // per tree: in-bag rows, open nodes per level, nodes
    int64_t g0, n_total;                // first tree of the batch, trees in the call
    // per workgroup (slot) of the batch
    int32_t *wy;                        // [n] weight * 2 + class
    int32_t *node_of;                   // [n] open node of the row at this level, -1
    uint8_t *side;                      // [n]
    Ent *S;                             // [2][d][cap_s]
    LNode *lvl;                         // [2][cap_lvl]
    NWork *work;                        // [cap_lvl]
    SBest *best;                        // [cap_lvl][d]
    FNode *nodes;                       // [cap_nodes]
    int32_t *n_nodes;                   // [batch]
    int *failed;
};

// exclusive prefix sum of v over the workgroup; every thread calls it; *total: the sum
__device__ __forceinline__ int block_scan(int v, int *tmp, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < NWAVE; ++w) {
        const int s = tmp[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

__device__ __forceinline__ double as_d(float x) { return (double)x; }

__global__ __launch_bounds__(BT) void k5_forest_fit(FitArgs A) {
    __shared__ int s_tmp[NWAVE];
    __shared__ unsigned long long s_sum[2];
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x, g = A.g0 + slot;
    if (g >= A.n_total) return;
    const int job = (int)(g / A.n_trees), t = (int)(g % A.n_trees);
    const FitJob J = A.jobs[job];
    const int d = A.d;
    const int64_t n = A.n, cap_s = A.cap_s, cap_lvl = A.cap_lvl;
    int32_t *wy = A.wy + slot * n;
    int32_t *node_of = A.node_of + slot * n;
    uint8_t *side = A.side + slot * n;
    Ent *S = A.S + slot * 2 * d * cap_s;
    LNode *lvl = A.lvl + slot * 2 * cap_lvl;
    NWork *work = A.work + slot * cap_lvl;
    SBest *best = A.best + slot * cap_lvl * d;
    FNode *nodes = A.nodes + slot * A.cap_nodes;
    const double *G = A.G;
    const float *Xt = A.Xt;

    // ---- bootstrap weights (draw counts) ----
    for (int64_t r = tid; r < n; r += BT) { wy[r] = 0; node_of[r] = -1; }
    __syncthreads();
    const uint64_t tk = splitmix64(J.seed + (uint64_t)(t + 1) * GOLD);
    const int32_t *tr = A.tr_idx + J.tr_off;
    for (int64_t i = tid; i < J.n_tr; i += BT) {
        int64_t pos = i;
        if (A.bootstrap) pos = (int64_t)(((splitmix64(tk + (uint64_t)i * DRAW) >> 32) * (uint64_t)J.n_tr) >> 32);
        atomicAdd(&wy[tr[pos]], 2);
    }
    __syncthreads();
    for (int64_t r = tid; r < n; r += BT)
        if (wy[r] > 0) wy[r] += A.y[r];
    if (tid < 2) s_sum[tid] = 0;
    __syncthreads();

    // ---- each feature's in-bag rows in sorted order (stable compaction of the presorted column) ----
    int n_s = 0;
    unsigned long long c0w = 0, c1w = 0;
    for (int f = 0; f < d; ++f) {
        Ent *Sf = S + (int64_t)f * cap_s;              // buffer 0
        const int32_t *of = A.order + (int64_t)f * n;
        int base = 0;
        for (int64_t p0 = 0; p0 < n; p0 += BT) {
            const int64_t p = p0 + tid;
            const int32_t r = p < n ? of[p] : -1;
            const int32_t v = r >= 0 ? wy[r] : 0;
            int tot;
            const int at = block_scan(v > 0 ? 1 : 0, s_tmp, &tot);
            if (v > 0) {
                Sf[base + at] = Ent{Xt[(int64_t)f * n + r], r};
                if (f == 0) {
                    node_of[r] = 0;
                    if (v & 1) c1w += (unsigned)(v >> 1); else c0w += (unsigned)(v >> 1);
                }
            }
            base += tot;
        }
        n_s = base;
    }
    atomicAdd(&s_sum[0], c0w);
    atomicAdd(&s_sum[1], c1w);
    __syncthreads();
    if (tid == 0) lvl[0] = LNode{0, n_s, (int32_t)s_sum[0], (int32_t)s_sum[1], 1ull};
    __syncthreads();

    // ---- level by level ----
    int cur = 0, n_cur = 1, n_out = 0;
    for (int depth = 0; n_cur > 0; ++depth) {
        LNode *L = lvl + (int64_t)cur * cap_lvl, *Lnext = lvl + (int64_t)(cur ^ 1) * cap_lvl;
        Ent *Sc = S + (int64_t)cur * d * cap_s, *Sn = S + (int64_t)(cur ^ 1) * d * cap_s;
        // (1) node records, leaf test, the features a node visits
        for (int k = tid; k < n_cur; k += BT) {
            const LNode nd = L[k];
            const int ns = nd.end - nd.start, W = nd.w0 + nd.w1;
            FNode o;
            o.left = -1; o.right = -1; o.feature = -2; o.n_samples = ns;
            o.threshold = -2.0;
            o.v0 = (double)nd.w0 / (double)W;
            o.v1 = (double)nd.w1 / (double)W;
            o.impurity = ((G[W] - G[nd.w0]) - G[nd.w1]) / ((double)W * LN2);
            o.weighted = (double)W;
            nodes[n_out + k] = o;
            NWork wk;
            wk.leaf = (depth >= A.max_depth || ns < A.mss || ns < 2 * A.msl || nd.w0 == 0 || nd.w1 == 0) ? 1 : 0;
            wk.nv = 0; wk.rank = -1; wk.feat = -1; wk.nleft = 0; wk.lbase = 0; wk.thr = -2.0;
            if (!wk.leaf) {
                const uint64_t nk = splitmix64(tk + nd.h * NODEK);
                int perm[DMAX];
                for (int i = 0; i < d; ++i) perm[i] = i;
                for (int i = d - 1; i >= 1; --i) {
                    const int j = (int)(((splitmix64(nk + (uint64_t)i) >> 32) * (uint64_t)(i + 1)) >> 32);
                    const int tmp = perm[i]; perm[i] = perm[j]; perm[j] = tmp;
                }
                int nv = 0, nc = 0;
                for (int j = 0; j < d; ++j) {
                    const int f = perm[j];
                    const Ent *Sf = Sc + (int64_t)f * cap_s;
                    const bool cst = as_d(Sf[nd.end - 1].x) <= as_d(Sf[nd.start].x) + (double)1e-7f;
                    nc += cst ? 1 : 0;
                    wk.vis[nv++] = (int8_t)(f + (cst ? 64 : 0));
                    if (!(nv < d && (nv < A.max_features || nv <= nc))) break;
                }
                wk.nv = nv;
            }
            work[k] = wk;
        }
        __syncthreads();
        // (2) a lane per (node, visited feature): the best split of that feature
        for (int64_t idx = tid; idx < (int64_t)n_cur * d; idx += BT) {
            const int k = (int)(idx / d), j = (int)(idx % d);
            const NWork &wk = work[k];
            if (wk.leaf || j >= wk.nv || wk.vis[j] >= 64) continue;
            const LNode nd = L[k];
            const int f = wk.vis[j];
            const Ent *Sf = Sc + (int64_t)f * cap_s;
            const int W0 = nd.w0, W1 = nd.w1, msl = A.msl, start = nd.start, end = nd.end;
            double bs = -INFINITY;
            int bp = -1, ba0 = 0, ba1 = 0;
            int a0 = 0, a1 = 0;
            Ent e = Sf[start];
            {
                const int v = wy[e.r];
                if (v & 1) a1 += v >> 1; else a0 += v >> 1;
            }
            double xprev = as_d(e.x);
            for (int p = start + 1; p < end; ++p) {
                e = Sf[p];
                const double xp = as_d(e.x);
                if (xp > xprev + (double)1e-7f && p - start >= msl && end - p >= msl) {
                    const int b0 = W0 - a0, b1 = W1 - a1;
                    const double s = ((G[a0] + G[a1]) - G[a0 + a1]) + ((G[b0] + G[b1]) - G[b0 + b1]);
                    if (s > bs) { bs = s; bp = p; ba0 = a0; ba1 = a1; }
                }
                const int v = wy[e.r];
                if (v & 1) a1 += v >> 1; else a0 += v >> 1;
                xprev = xp;
            }
            best[(int64_t)k * d + j] = SBest{bs, bp, ba0, ba1, 0};
        }
        __syncthreads();
        // (3) a lane per node: the best over its features; ranks of the split nodes, where their left rows start in a list
        int n_split = 0, left_base = 0;
        for (int c0 = 0; c0 < n_cur; c0 += BT) {
            const int k = c0 + tid;
            int split = 0, nleft = 0;
            if (k < n_cur) {
                NWork &wk = work[k];
                if (!wk.leaf) {
                    double bs = -INFINITY;
                    int bj = -1;
                    for (int j = 0; j < wk.nv; ++j) {
                        if (wk.vis[j] >= 64) continue;
                        const SBest &b = best[(int64_t)k * d + j];
                        if (b.pos >= 0 && b.score > bs) { bs = b.score; bj = j; }
                    }
                    if (bj >= 0) {
                        const LNode nd = L[k];
                        const SBest b = best[(int64_t)k * d + bj];
                        const int f = wk.vis[bj];
                        const Ent *Sf = Sc + (int64_t)f * cap_s;
                        const double xa = as_d(Sf[b.pos - 1].x), xb = as_d(Sf[b.pos].x);
                        double th = xa / 2.0 + xb / 2.0;
                        if (th == xb || isinf(th)) th = xa;
                        wk.feat = f; wk.thr = th; wk.nleft = b.pos - nd.start;
                        split = 1; nleft = wk.nleft;
                        best[(int64_t)k * d] = b;          // (slot 0 keeps the chosen split's class weights)
                    }
                }
            }
            int tot_s, tot_l;
            const int rank = block_scan(split, s_tmp, &tot_s);
            const int lb = block_scan(nleft, s_tmp, &tot_l);
            if (split) {
                NWork &wk = work[k];
                wk.rank = n_split + rank;
                wk.lbase = left_base + lb;
                const LNode nd = L[k];
                const SBest b = best[(int64_t)k * d];
                const int r2 = 2 * wk.rank;
                if (r2 + 1 < cap_lvl) {
                    Lnext[r2] = LNode{nd.start, nd.start + wk.nleft, b.a0, b.a1, 2 * nd.h};
                    Lnext[r2 + 1] = LNode{nd.start + wk.nleft, nd.end, nd.w0 - b.a0, nd.w1 - b.a1, 2 * nd.h + 1};
                } else {
                    *A.failed = 1;
                }
                FNode &o = nodes[n_out + k];
                o.feature = wk.feat;
                o.threshold = wk.thr;
                o.left = n_out + n_cur + r2;
                o.right = n_out + n_cur + r2 + 1;
            }
            n_split += tot_s;
            left_base += tot_l;
        }
        __syncthreads();
        const int n_next = 2 * n_split;
        if (n_out + n_cur + n_next > A.cap_nodes || n_next > cap_lvl) {        // (cannot happen: the capacities are bounds)
            if (tid == 0) *A.failed = 1;
            n_out += n_cur;
            break;
        }
        if (n_split > 0) {
            // (4) the side of every row of a split node
            const Ent *S0 = Sc;
            for (int p = tid; p < n_s; p += BT) {
                const int32_t r = S0[p].r;
                const int k = node_of[r];
                if (k < 0) continue;
                const NWork &wk = work[k];
                if (wk.rank >= 0) side[r] = (as_d(Xt[(int64_t)wk.feat * n + r]) <= wk.thr) ? 0 : 1;
            }
            __syncthreads();
            // (5) every feature's list stable-partitioned: left rows, then right rows, inside each split node's segment
            for (int f = 0; f < d; ++f) {
                const Ent *Sf = Sc + (int64_t)f * cap_s;
                Ent *Df = Sn + (int64_t)f * cap_s;
                int base = 0;
                for (int p0 = 0; p0 < n_s; p0 += BT) {
                    const int p = p0 + tid;
                    Ent e{0.f, -1};
                    int k = -1, rank = -1, sd = 1;
                    if (p < n_s) {
                        e = Sf[p];
                        k = node_of[e.r];
                        if (k >= 0) {
                            rank = work[k].rank;
                            if (rank >= 0) sd = side[e.r];
                        }
                    }
                    const int isl = (rank >= 0 && sd == 0) ? 1 : 0;
                    int tot;
                    const int lpre = base + block_scan(isl, s_tmp, &tot);
                    if (p < n_s) {
                        int np = p;
                        if (rank >= 0) {
                            const NWork &wk = work[k];
                            const int start = L[k].start;
                            const int lr = lpre - wk.lbase;
                            np = isl ? start + lr : start + wk.nleft + (p - start - lr);
                        }
                        Df[np] = e;
                    }
                    base += tot;
                }
            }
            __syncthreads();
            // (6) the rows' nodes at the next level
            for (int p = tid; p < n_s; p += BT) {
                const int32_t r = Sn[p].r;
                const int k = node_of[r];
                if (k < 0) continue;
                const int rank = work[k].rank;
                node_of[r] = rank >= 0 ? 2 * rank + side[r] : -1;
            }
            __syncthreads();
        }
        n_out += n_cur;
        n_cur = n_next;
        cur ^= 1;
    }
    if (tid == 0) A.n_nodes[slot] = n_out;
}

struct ValArgs {
    const double *X;
    const uint8_t *y;
    const int32_t *va_idx;
    const FitJob *jobs;
    const int64_t *tree_node_off;       // [n_jobs * n_trees + 1], absolute
    const int32_t *left, *right, *feature;
    const double *threshold, *value;
    int32_t d, n_trees;
    unsigned long long *val_correct;
};

// a lane per validation row of a job (grid.y: job): P_c = sum over trees, in tree order, of v_c / ((-0.0 + v0) + v1), over n_trees
__global__ __launch_bounds__(256) void k5_forest_val(ValArgs A) {
    const int job = blockIdx.y;
    const FitJob J = A.jobs[job];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int ok = 0;
    if (i < J.n_va) {
        const int32_t row = A.va_idx[J.va_off + i];
        double x[DMAX];
        for (int f = 0; f < A.d; ++f) x[f] = (double)(float)A.X[(int64_t)row * A.d + f];
        double P0 = 0.0, P1 = 0.0;
        for (int t = 0; t < A.n_trees; ++t) {
            int64_t node = A.tree_node_off[(int64_t)job * A.n_trees + t];
            const int64_t base = node;
            int l;
            while ((l = A.left[node]) >= 0) node = base + ((x[A.feature[node]] <= A.threshold[node]) ? l : A.right[node]);
            const double v0 = A.value[2 * node], v1 = A.value[2 * node + 1];
            double norm = (-0.0 + v0) + v1;
            if (norm == 0.0) norm = 1.0;
            P0 += v0 / norm;
            P1 += v1 / norm;
        }
        P0 /= (double)A.n_trees;
        P1 /= (double)A.n_trees;
        ok = ((P1 > P0 ? 1 : 0) == (int)A.y[row]) ? 1 : 0;
    }
    // (integer additions: the count does not depend on their order)
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&A.val_correct[job], (unsigned long long)__popcll(m));
}

}  // namespace

extern "C" int mc_forest_fit(mc_ctx *c, const mc_forest_params *P, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_jobs,
                             const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx,
                             const uint64_t *seeds, const double *G, int64_t n_G, int64_t node_cap, int64_t *tree_node_off,
                             int32_t *left, int32_t *right, int32_t *feature, double *threshold, double *value, double *impurity,
                             int32_t *n_node_samples, double *weighted_n_node_samples, int64_t *val_correct) {
    if (!P || !X || !y || !train_off || !train_idx || !val_off || !seeds || !G || !tree_node_off || !left || !right || !feature ||
        !threshold || !value || !impurity || !n_node_samples || !weighted_n_node_samples || !val_correct) {
        mc_set_error("mc_forest_fit: a required pointer is NULL");
        return -12;
    }
    const int d = P->n_in;
    if (d < 1 || d > DMAX) { mc_set_error("mc_forest_fit: n_in %d out of range 1..%d", d, DMAX); return -12; }
    if (P->n_trees < 1 || P->n_trees > 100000) { mc_set_error("mc_forest_fit: n_trees %d out of range 1..100000", P->n_trees); return -12; }
    if (P->max_depth < 1 || P->max_depth > 30) { mc_set_error("mc_forest_fit: max_depth %d out of range 1..30", P->max_depth); return -12; }
    if (P->max_features < 1 || P->max_features > d) {
        mc_set_error("mc_forest_fit: max_features must be in (0, n_features]: %d with %d features", P->max_features, d);
        return -12;
    }
    if (P->min_samples_split < 2) { mc_set_error("mc_forest_fit: min_samples_split %d < 2", P->min_samples_split); return -12; }
    if (P->min_samples_leaf < 1) { mc_set_error("mc_forest_fit: min_samples_leaf %d < 1", P->min_samples_leaf); return -12; }
    if (P->bootstrap != 0 && P->bootstrap != 1) { mc_set_error("mc_forest_fit: bootstrap must be 0 or 1"); return -12; }
    if (n_samples < 1 || n_samples > ((int64_t)1 << 28) || n_jobs < 1 || (int64_t)n_jobs * P->n_trees > ((int64_t)1 << 31)) {
        mc_set_error("mc_forest_fit: %lld samples, %d jobs out of range", (long long)n_samples, n_jobs);
        return -12;
    }
    if (int rc = check_jobs("mc_forest_fit", X, y, n_samples, d, n_jobs, train_off, train_idx, val_off, val_idx, (int64_t)1 << 28, 1, false, true, nullptr))
        return rc;
    int64_t max_tr = 0, max_va = 0, need_nodes = 0;
    const int64_t depth_nodes = ((int64_t)2 << P->max_depth) - 1;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t ntr = train_off[j + 1] - train_off[j];
        max_tr = std::max(max_tr, ntr);
        max_va = std::max(max_va, val_off[j + 1] - val_off[j]);
        need_nodes += (int64_t)P->n_trees * std::min(depth_nodes, 2 * ntr - 1);
    }
    if (n_G < max_tr + 1) { mc_set_error("mc_forest_fit: G table of %lld entries, %lld needed", (long long)n_G, (long long)(max_tr + 1)); return -12; }
    if (node_cap < need_nodes) { mc_set_error("mc_forest_fit: node_cap %lld < %lld", (long long)node_cap, (long long)need_nodes); return -12; }
    if (int rc = select_device("mc_forest_fit", c)) return rc;
    const int64_t n = n_samples, T = P->n_trees, total = (int64_t)n_jobs * T;

    // host: float32 columns and each column's row order (stable: rows in index order among equal values)
    std::vector<float> Xt((size_t)d * n);
    for (int64_t i = 0; i < n; ++i)
        for (int f = 0; f < d; ++f) Xt[(size_t)f * n + i] = (float)X[i * d + f];
    std::vector<int32_t> order((size_t)d * n);
    for (int f = 0; f < d; ++f) {
        int32_t *o = order.data() + (size_t)f * n;
        std::iota(o, o + n, 0);
        const float *col = Xt.data() + (size_t)f * n;
        std::stable_sort(o, o + n, [col](int32_t a, int32_t b) { return col[a] < col[b]; });
    }
    std::vector<FitJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j)
        jobs[j] = FitJob{train_off[j], train_off[j + 1] - train_off[j], val_off[j], val_off[j + 1] - val_off[j], seeds[j]};

    const int64_t cap_s = max_tr;
    const int64_t cap_lvl = std::max<int64_t>(2, std::min<int64_t>((int64_t)1 << P->max_depth, cap_s) + 1);
    const int64_t cap_nodes = std::min(depth_nodes, 2 * cap_s - 1);
    const size_t per_tree = (size_t)n * (4 + 4 + 1) + (size_t)2 * d * cap_s * sizeof(Ent) + (size_t)cap_lvl * (2 * sizeof(LNode) + sizeof(NWork) + d * sizeof(SBest)) +
                            (size_t)cap_nodes * sizeof(FNode) + 64;
    static const int64_t budget_mb = getenv("MCALLER_FOREST_MEM_MB") ? atoll(getenv("MCALLER_FOREST_MEM_MB")) : 4096;
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(total, (std::max<int64_t>(budget_mb, 1) << 20) / (int64_t)per_tree));
    mc_forest_fit_stats &stats = *mc_internal_forest_stats(c);
    stats = mc_forest_fit_stats{(total + batch - 1) / batch, batch, (int64_t)per_tree, total, 0};

    const int64_t n_tr = train_off[n_jobs], n_va = val_off[n_jobs];
    Pool pool("mc_forest_fit");
    FitArgs A;
    float *dXt = pool.get<float>((size_t)d * n);
    int32_t *dorder = pool.get<int32_t>((size_t)d * n);
    uint8_t *dy = pool.get<uint8_t>((size_t)n);
    int32_t *dtr = pool.get<int32_t>((size_t)n_tr), *dva = pool.get<int32_t>((size_t)n_va);
    FitJob *djobs = pool.get<FitJob>((size_t)n_jobs);
    double *dG = pool.get<double>((size_t)n_G);
    double *dX = pool.get<double>((size_t)n * d);
    A.wy = pool.get<int32_t>((size_t)batch * n);
    A.node_of = pool.get<int32_t>((size_t)batch * n);
    A.side = pool.get<uint8_t>((size_t)batch * n);
    A.S = pool.get<Ent>((size_t)batch * 2 * d * cap_s);
    A.lvl = pool.get<LNode>((size_t)batch * 2 * cap_lvl);
    A.work = pool.get<NWork>((size_t)batch * cap_lvl);
    A.best = pool.get<SBest>((size_t)batch * cap_lvl * d);
    A.nodes = pool.get<FNode>((size_t)batch * cap_nodes);
    A.n_nodes = pool.get<int32_t>((size_t)batch);
    A.failed = pool.get<int>(1);
    unsigned long long *dcorrect = pool.get<unsigned long long>((size_t)n_jobs);
    if (!pool.ok) return -10;
    Xfer x("mc_forest_fit", mc_internal_stream(c));
    x.up(dXt, Xt.data(), Xt.size());
    x.up(dorder, order.data(), order.size());
    x.up(dy, y, (size_t)n);
    x.up(dtr, train_idx, (size_t)n_tr);
    x.up(dva, val_idx, (size_t)n_va);
    x.up(djobs, jobs.data(), jobs.size());
    x.up(dG, G, (size_t)n_G);
    x.up(dX, X, (size_t)n * d);
    x.zero(A.failed, 1);
    x.zero(dcorrect, (size_t)n_jobs);
    A.Xt = dXt; A.order = dorder; A.y = dy; A.tr_idx = dtr; A.jobs = djobs; A.G = dG;
    A.d = d; A.n_trees = P->n_trees; A.max_depth = P->max_depth; A.max_features = P->max_features;
    A.mss = P->min_samples_split; A.msl = P->min_samples_leaf; A.bootstrap = P->bootstrap;
    A.n = n; A.cap_s = cap_s; A.cap_lvl = cap_lvl; A.cap_nodes = cap_nodes; A.n_total = total;

    // grow the trees batch by batch; each batch's level-order nodes renumbered into pre-order on the host
    std::vector<FNode> hn((size_t)batch * cap_nodes);
    std::vector<int32_t> hcount((size_t)batch);
    std::vector<int32_t> stack, newid;
    int64_t out = 0;
    tree_node_off[0] = 0;
    for (int64_t g0 = 0; g0 < total && x.ok(); g0 += batch) {
        const int64_t nb = std::min(batch, total - g0);
        A.g0 = g0;
        x.launch(k5_forest_fit, dim3((unsigned)nb), dim3(BT), 0, A);
        x.down(hcount.data(), A.n_nodes, (size_t)nb);
        x.sync();
        for (int64_t b = 0; b < nb && x.ok(); ++b) {
            const int cnt = hcount[b];
            if (cnt < 1 || cnt > cap_nodes || out + cnt > node_cap) {
                mc_set_error("mc_forest_fit: tree %lld came back with %d nodes", (long long)(g0 + b), cnt);
                return -10;
            }
            x.down(hn.data() + b * cap_nodes, A.nodes + b * cap_nodes, (size_t)cnt);
        }
        x.sync();
        for (int64_t b = 0; b < nb && x.ok(); ++b) {
            const FNode *tn = hn.data() + b * cap_nodes;
            const int cnt = hcount[b];
            newid.assign((size_t)cnt, -1);
            stack.assign(1, 0);
            int next = 0;
            while (!stack.empty()) {                       // depth-first, left before right
                const int v = stack.back();
                stack.pop_back();
                newid[v] = next++;
                if (tn[v].left >= 0) {
                    if (tn[v].left >= cnt || tn[v].right >= cnt) { mc_set_error("mc_forest_fit: a child link out of range"); return -10; }
                    stack.push_back(tn[v].right);
                    stack.push_back(tn[v].left);
                }
            }
            if (next != cnt) { mc_set_error("mc_forest_fit: tree %lld is not connected", (long long)(g0 + b)); return -10; }
            for (int v = 0; v < cnt; ++v) {
                const int64_t o = out + newid[v];
                const FNode &s = tn[v];
                left[o] = s.left >= 0 ? newid[s.left] : -1;
                right[o] = s.right >= 0 ? newid[s.right] : -1;
                feature[o] = s.feature;
                threshold[o] = s.threshold;
                value[2 * o] = s.v0;
                value[2 * o + 1] = s.v1;
                impurity[o] = s.impurity;
                n_node_samples[o] = s.n_samples;
                weighted_n_node_samples[o] = s.weighted;
            }
            out += cnt;
            tree_node_off[g0 + b + 1] = out;
        }
    }
    int failed = 0;
    x.down(&failed, A.failed, 1);
    x.sync();
    if (x.ok() && failed) { mc_set_error("mc_forest_fit: a tree outgrew its work arrays"); return -10; }

    // validation: each job's rows scored by its own trees (the trees in pre-order, local child links)
    if (x.ok()) {
        int64_t *dtoff = pool.get<int64_t>((size_t)total + 1);
        int32_t *dl = pool.get<int32_t>((size_t)out), *dr = pool.get<int32_t>((size_t)out), *df = pool.get<int32_t>((size_t)out);
        double *dth = pool.get<double>((size_t)out), *dv = pool.get<double>((size_t)out * 2);
        if (!pool.ok) return -10;
        x.up(dtoff, tree_node_off, (size_t)total + 1);
        x.up(dl, left, (size_t)out);
        x.up(dr, right, (size_t)out);
        x.up(df, feature, (size_t)out);
        x.up(dth, threshold, (size_t)out);
        x.up(dv, value, (size_t)out * 2);
        if (max_va > 0)
            x.launch(k5_forest_val, dim3((unsigned)((max_va + 255) / 256), (unsigned)n_jobs), dim3(256), 0,
                     ValArgs{dX, dy, dva, djobs, dtoff, dl, dr, df, dth, dv, d, P->n_trees, dcorrect});
        x.down(val_correct, dcorrect, (size_t)n_jobs);
        x.sync();
    }
    if (!x.ok()) return x.fail();
    stats.n_nodes = out;
    return 0;
}

extern "C" int mc_forest_fit_last_stats(mc_ctx *c, mc_forest_fit_stats *out) {
    if (!c || !out) { mc_set_error("mc_forest_fit_last_stats: bad arguments"); return -12; }
    *out = *mc_internal_forest_stats(c);
    return 0;
}
