// libmcaller_hip.so -- the closed-form classifiers' fits behind `--train -c LR` and `--train -c NBC` on the GPU (gfx950 / MI355X).
// C ABI: include/mcaller_hip.h.  Scored afterwards by k3_simple (mc_classify.hip), hence the unit's name.
//
// The reference fits LogisticRegression(solver='liblinear', penalty='l1') or GaussianNB() per sub-model, five times for GroupKFold and
// once more on all rows (train_model.py:55-60,:62-65,:92-101).  Every fit is one workgroup of one launch; no workgroup waits for
// another.  fp64 throughout.
//
// k7_lr_fit is liblinear's solve_l1r_lr (newGLMNET) as scikit-learn vendors it (tests/lr_fit_oracle.py restates it in NumPy):
//   * The job's training rows are copied into a column-major block, classes_[0] rows first (y = -1), the bias column of 1.0 last.
//   * A lane owns the rows t = tid + BT r: exp_wTx, exp_wTx_new, tau, D and xTd live in global memory (L2-resident at these sizes)
//     and only the owner reads or writes them, so the block reductions are the only barriers.
//   * Thread 0 runs liblinear's control flow on the per-feature state in LDS (w, wpd, Grad, Hdiag, the active-set index and the
//     std::mt19937 of the QP shuffle, seeded once per fit); the other lanes do the row passes it asks for.  A Newton iteration is
//     one multi-value reduction (Grad and Hdiag of every feature), then one reduction per coordinate step (the step's xTd update
//     is applied by the owners in the next pass over the rows), then one per line-search step.
//   * Reductions run in a fixed order (a lane's rows in order, a butterfly over the wave, the waves in order): two identical calls
//     give identical bytes.  The sums differ in order from liblinear's row walk, so the device's w agrees with the oracle's within
//     the solver's tolerance, not bit for bit.
//   * Then the same workgroup scores its held-out rows with k3_simple's arithmetic (dot product in index order, plus the intercept).
// k7_nb_fit is GaussianNB's fit: per class the counts, means and centred (two-pass) variances, epsilon_ = var_smoothing times the
// largest per-feature variance of the job's rows, added to every variance; then the held-out rows scored as k3_simple does.
// The entry points' allocations, transfers and job checks, FitJob, splitmix64 and wave_sum: mc_fit.h.
#include "mc_fit.h"

namespace {

constexpr int BT = 512;                         // threads per fit (1024 would cap a lane at 128 VGPRs: spills)
constexpr int NWAVE = BT / 64;
constexpr int DMAX = 64;                        // features
constexpr int NMAX = DMAX + 1;                  // and the bias
constexpr int MAX_INNER = 1000, MAX_LINESEARCH = 20;
constexpr double NU = 1e-12, SIGMA = 0.01;
constexpr int64_t MAX_ROWS = (int64_t)1 << 26;  // per job and per call
constexpr int64_t MEM_CAP = (int64_t)4 << 30;   // device work memory of one call, bytes

struct Job {
    int64_t tr_off, n_tr, n_neg, va_off, n_va;  // n_neg: classes_[0] rows, the first of the job's rows
    uint32_t seed;
    int32_t pad;
};

struct LrArgs {
    const double *X;                            // [n][d]
    const uint8_t *y;
    const int32_t *tr_idx;                      // per job, classes_[0] rows first, at tr_off
    const int32_t *va_idx;
    const Job *jobs;
    double *Xc;                                 // per job [d+1][n_tr], at tr_off * (d+1)
    double *ew, *ewn, *tau, *D, *xTd;           // per row, at tr_off
    int d, max_iter;
    double C, tol;
    double *w;                                  // per job [d+1], the bias last
    int *n_iter, *status;
    double *dec;                                // at va_off
    long long *correct;
};

struct NbArgs {
    const double *X;
    const uint8_t *y;
    const int32_t *tr_idx, *va_idx;
    const Job *jobs;
    int d;
    double var_smoothing;
    double *theta, *var;                        // per job [2][d]
    double *epsilon;
    long long *correct;
};

// std::mt19937 (seed(s), operator()) and scikit-learn's bounded_rand_int (newrand.h: Lemire's method, the low word below
// 2^32 mod range redrawn); one lane uses it
struct MT {
    uint32_t s[624];
    int i;
};

__device__ void mt_seed(MT &m, uint32_t seed) {
    m.s[0] = seed;
    for (int k = 1; k < 624; ++k) m.s[k] = 1812433253u * (m.s[k - 1] ^ (m.s[k - 1] >> 30)) + (uint32_t)k;
    m.i = 624;
}

__device__ uint32_t mt_next(MT &m) {
    if (m.i >= 624) {
        for (int k = 0; k < 624; ++k) {
            const uint32_t y = (m.s[k] & 0x80000000u) | (m.s[k + 1 < 624 ? k + 1 : 0] & 0x7fffffffu);
            m.s[k] = m.s[k + 397 < 624 ? k + 397 : k + 397 - 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        m.i = 0;
    }
    uint32_t y = m.s[m.i++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

__device__ uint32_t bounded_rand(MT &m, uint32_t range) {
    uint64_t p = (uint64_t)mt_next(m) * range;
    uint32_t lo = (uint32_t)p;
    if (lo < range) {
        const uint32_t t = (0u - range) % range;
        while (lo < t) {
            p = (uint64_t)mt_next(m) * range;
            lo = (uint32_t)p;
        }
    }
    return (uint32_t)(p >> 32);
}

__device__ __forceinline__ void iswap(int &a, int &b) {
    const int t = a;
    a = b;
    b = t;
}

// np.sum of n <= 128 doubles as numpy adds them (pairwise_sum): in order below 8 terms; from 8 on, eight partial sums, then
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and the rest in order -- k3_simple's np_row_sum, for any n_in
template <typename F>
__device__ double np_sum(int n, F f) {
    if (n < 8) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += f(i);
        return s;
    }
    double r0 = f(0), r1 = f(1), r2 = f(2), r3 = f(3), r4 = f(4), r5 = f(5), r6 = f(6), r7 = f(7);
    int i = 8;
    for (; i + 8 <= n; i += 8) {
        r0 += f(i); r1 += f(i + 1); r2 += f(i + 2); r3 += f(i + 3);
        r4 += f(i + 4); r5 += f(i + 5); r6 += f(i + 6); r7 += f(i + 7);
    }
    double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) s += f(i);
    return s;
}

__global__ __launch_bounds__(BT) void k7_lr_fit(LrArgs A) {
    __shared__ double s_w[NMAX], s_wpd[NMAX], s_grad[NMAX], s_hdiag[NMAX], s_xneg[NMAX];
    __shared__ double s_red[NWAVE][NMAX][2];
    __shared__ double s_part[NWAVE], s_pz;
    __shared__ long long s_cnt[NWAVE];
    __shared__ int s_idx[NMAX], s_j, s_pj, s_flag;
    __shared__ MT s_mt;

    const Job J = A.jobs[blockIdx.x];
    const int64_t l = J.n_tr, nneg = J.n_neg;
    const double dl = (double)l;
    const int d = A.d, n = d + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *Xc = A.Xc + J.tr_off * n;
    double *ew = A.ew + J.tr_off, *ewn = A.ewn + J.tr_off, *tau = A.tau + J.tr_off, *D = A.D + J.tr_off, *xTd = A.xTd + J.tr_off;
    const int32_t *tr = A.tr_idx + J.tr_off;
    const double C = A.C;

    // the block's sum of one value per lane, every lane leaving with it (s_part: written before the barrier, read after it; the
    // next write comes after another barrier)
    auto block_sum = [&](double v) {
        v = wave_sum(v);
        if (lane == 0) s_part[wave] = v;
        __syncthreads();
        double s = 0.0;
        for (int w = 0; w < NWAVE; ++w) s += s_part[w];
        __syncthreads();
        return s;
    };
    // per column j < n two sums over the rows (term(j, t, a, b) adds row t's); thread j < n reads them from s_red after the barrier
    auto reduce_cols = [&](auto &&term) {
        for (int j = 0; j < n; ++j) {
            double a = 0.0, b = 0.0;
            for (int64_t t = tid; t < l; t += BT) term(j, t, a, b);
            a = wave_sum(a);
            b = wave_sum(b);
            if (lane == 0) { s_red[wave][j][0] = a; s_red[wave][j][1] = b; }
        }
        __syncthreads();
    };

    // the job's rows, column-major, the bias column last; w = 0: exp_wTx = 1 (linear.cpp:1801-1845)
    for (int64_t t = tid; t < l; t += BT) {
        const double *x = A.X + (int64_t)tr[t] * d;
        for (int f = 0; f < d; ++f) Xc[f * l + t] = x[f];
        Xc[d * l + t] = 1.0;
        const double e = 1.0, tt = 1.0 / (1.0 + e);
        ew[t] = e;
        tau[t] = C * tt;
        D[t] = C * e * tt * tt;
        xTd[t] = 0.0;
    }
    reduce_cols([&](int j, int64_t t, double &a, double &) { if (t < nneg) a += C * Xc[j * l + t]; });
    if (tid < n) {
        double s = 0.0;
        for (int w = 0; w < NWAVE; ++w) s += s_red[w][tid][0];
        s_xneg[tid] = s;
        s_w[tid] = 0.0;
        s_wpd[tid] = 0.0;
        s_idx[tid] = tid;
    }
    if (tid == 0) {
        mt_seed(s_mt, J.seed);
        s_pj = -1;
        s_pz = 0.0;
    }
    __syncthreads();

    // thread 0's state (liblinear's scalars)
    const int pos = (int)(l - nneg);
    const double eps = A.tol * (double)std::max(std::min<int64_t>(pos, nneg), (int64_t)1) / dl;
    double Gmax_old = INFINITY, Gmax_new = 0.0, inner_eps = 1.0, Gnorm1_init = -1.0, w_norm = 0.0, w_norm_new = 0.0, delta = 0.0;
    double QP_Gmax_old = INFINITY, QP_Gmax_new = 0.0, QP_Gnorm1_new = 0.0;
    int QP_no_change = 0, active_size = n, QP_active_size = n, s = 0;

    int newton_iter = 0;
    while (newton_iter < A.max_iter) {
        // Grad and Hdiag of every feature (:1853-1868), then the outer pass with its shrinking (:1869-1895) on thread 0
        reduce_cols([&](int j, int64_t t, double &a, double &b) {
            const double x = Xc[j * l + t];
            a += x * x * D[t];
            b += x * tau[t];
        });
        if (tid < n) {
            double h = NU, g = 0.0;
            for (int w = 0; w < NWAVE; ++w) { h += s_red[w][tid][0]; g += s_red[w][tid][1]; }
            s_hdiag[tid] = h;
            s_grad[tid] = -g + s_xneg[tid];
        }
        __syncthreads();
        if (tid == 0) {
            double Gnorm1_new = 0.0;
            Gmax_new = 0.0;
            active_size = n;
            for (int k = 0; k < active_size;) {
                const int j = s_idx[k];
                const double Gp = s_grad[j] + 1, Gn = s_grad[j] - 1, wj = s_w[j];
                double violation = 0.0;
                if (wj == 0) {
                    if (Gp < 0) violation = -Gp;
                    else if (Gn > 0) violation = Gn;
                    else if (Gp > Gmax_old / dl && Gn < -Gmax_old / dl) {
                        --active_size;
                        iswap(s_idx[k], s_idx[active_size]);
                        continue;
                    }
                } else if (wj > 0) violation = fabs(Gp);
                else violation = fabs(Gn);
                Gmax_new = fmax(Gmax_new, violation);
                Gnorm1_new += violation;
                ++k;
            }
            if (newton_iter == 0) Gnorm1_init = Gnorm1_new;
            const bool stop = Gnorm1_new <= eps * Gnorm1_init || QP_no_change >= 10;
            s_flag = stop ? 1 : 0;
            if (!stop) {
                ++QP_no_change;
                QP_Gmax_old = INFINITY;
                QP_active_size = active_size;
            }
        }
        __syncthreads();
        if (s_flag) break;
        for (int64_t t = tid; t < l; t += BT) xTd[t] = 0.0;

        // coordinate descent on the quadratic model (:1915-2007)
        int iter = 0;
        while (iter < MAX_INNER) {
            if (tid == 0) {
                QP_Gmax_new = 0.0;
                QP_Gnorm1_new = 0.0;
                for (int k = 0; k < QP_active_size; ++k) {
                    const int i = k + (int)bounded_rand(s_mt, (uint32_t)(QP_active_size - k));
                    iswap(s_idx[i], s_idx[k]);
                }
                s = 0;
                s_j = QP_active_size > 0 ? s_idx[0] : -1;
            }
            __syncthreads();
            for (;;) {
                const int j = s_j, pj = s_pj;
                const double pz = s_pz;
                if (j < 0) break;
                const double *xj = Xc + (int64_t)j * l, *xp = Xc + (int64_t)(pj >= 0 ? pj : 0) * l;
                double part = 0.0;
                for (int64_t t = tid; t < l; t += BT) {
                    double v = xTd[t];
                    if (pj >= 0) { v += xp[t] * pz; xTd[t] = v; }          // the previous step's update (:1981-1987)
                    part += xj[t] * D[t] * v;
                }
                part = wave_sum(part);
                if (lane == 0) s_part[wave] = part;
                __syncthreads();
                if (tid == 0) {
                    double sum = 0.0;
                    for (int w = 0; w < NWAVE; ++w) sum += s_part[w];
                    const double H = s_hdiag[j], wpd = s_wpd[j];
                    const double G = s_grad[j] + (wpd - s_w[j]) * NU + sum;
                    const double Gp = G + 1, Gn = G - 1;
                    double violation = 0.0;
                    bool shrink = false;
                    if (wpd == 0) {
                        if (Gp < 0) violation = -Gp;
                        else if (Gn > 0) violation = Gn;
                        else if (Gp > QP_Gmax_old / dl && Gn < -QP_Gmax_old / dl) shrink = true;
                    } else if (wpd > 0) violation = fabs(Gp);
                    else violation = fabs(Gn);
                    s_pj = -1;
                    if (shrink) {
                        --QP_active_size;
                        iswap(s_idx[s], s_idx[QP_active_size]);
                    } else {
                        double z;
                        if (Gp < H * wpd) z = -Gp / H;
                        else if (Gn > H * wpd) z = -Gn / H;
                        else z = -wpd;
                        if (fabs(z) >= 1.0e-12) {
                            z = fmin(fmax(z, -10.0), 10.0);
                            QP_no_change = 0;
                            QP_Gmax_new = fmax(QP_Gmax_new, violation);
                            QP_Gnorm1_new += violation;
                            s_wpd[j] = wpd + z;
                            s_pj = j;
                            s_pz = z;
                        }
                        ++s;
                    }
                    s_j = s < QP_active_size ? s_idx[s] : -1;
                }
                __syncthreads();
            }
            ++iter;
            if (tid == 0) {
                int brk = 0;
                if (QP_Gnorm1_new <= inner_eps * Gnorm1_init) {
                    if (QP_active_size == active_size) brk = 1;
                    else { QP_active_size = active_size; QP_Gmax_old = INFINITY; }
                } else {
                    QP_Gmax_old = QP_Gmax_new;
                }
                s_flag = brk;
            }
            __syncthreads();
            if (s_flag) break;
        }

        // the line search (:2012-2067): the pending xTd update first, with negsum_xTd
        {
            const int pj = s_pj;
            const double pz = s_pz;
            const double *xp = Xc + (int64_t)(pj >= 0 ? pj : 0) * l;
            double part = 0.0;
            for (int64_t t = tid; t < l; t += BT) {
                double v = xTd[t];
                if (pj >= 0) { v += xp[t] * pz; xTd[t] = v; }
                if (t < nneg) part += C * v;
            }
            const double negsum0 = block_sum(part);
            if (tid == 0) {
                s_pj = -1;
                delta = 0.0;
                w_norm_new = 0.0;
                for (int j = 0; j < n; ++j) {
                    delta += s_grad[j] * (s_wpd[j] - s_w[j]);
                    if (s_wpd[j] != 0) w_norm_new += fabs(s_wpd[j]);
                }
                delta += w_norm_new - w_norm;
            }
            double negsum = negsum0;                // (thread 0's copy is the one used)
            int num_linesearch = 0;
            for (; num_linesearch < MAX_LINESEARCH; ++num_linesearch) {
                double p2 = 0.0;
                for (int64_t t = tid; t < l; t += BT) {
                    const double exd = exp(xTd[t]), e = ew[t] * exd;
                    ewn[t] = e;
                    p2 += C * log((1 + e) / (exd + e));
                }
                p2 = wave_sum(p2);
                if (lane == 0) s_part[wave] = p2;
                __syncthreads();
                if (tid == 0) {
                    double sum = 0.0;
                    for (int w = 0; w < NWAVE; ++w) sum += s_part[w];
                    const double cond = w_norm_new - w_norm + negsum - SIGMA * delta + sum;
                    if (cond <= 0) {
                        w_norm = w_norm_new;
                        for (int j = 0; j < n; ++j) s_w[j] = s_wpd[j];
                        s_flag = 1;
                    } else {
                        w_norm_new = 0.0;
                        for (int j = 0; j < n; ++j) {
                            s_wpd[j] = (s_w[j] + s_wpd[j]) * 0.5;
                            if (s_wpd[j] != 0) w_norm_new += fabs(s_wpd[j]);
                        }
                        delta *= 0.5;
                        negsum *= 0.5;
                        s_flag = 0;
                    }
                }
                __syncthreads();
                if (s_flag) {
                    for (int64_t t = tid; t < l; t += BT) {
                        const double e = ewn[t], tt = 1 / (1 + e);
                        ew[t] = e;
                        tau[t] = C * tt;
                        D[t] = C * e * tt * tt;
                    }
                    break;
                }
                for (int64_t t = tid; t < l; t += BT) xTd[t] *= 0.5;
            }
            if (num_linesearch >= MAX_LINESEARCH) {  // (:2070-2088: exp_wTx again from w; tau and D stay)
                for (int64_t t = tid; t < l; t += BT) {
                    double a = 0.0;
                    for (int i = 0; i < n; ++i)
                        if (s_w[i] != 0) a += s_w[i] * Xc[(int64_t)i * l + t];
                    ew[t] = exp(a);
                }
            }
        }
        if (tid == 0) {
            if (iter == 1) inner_eps *= 0.25;
            Gmax_old = Gmax_new;
        }
        ++newton_iter;
        __syncthreads();
    }

    if (tid < n) A.w[(int64_t)blockIdx.x * n + tid] = s_w[tid];
    if (tid == 0) {
        A.n_iter[blockIdx.x] = newton_iter;
        A.status[blockIdx.x] = newton_iter >= A.max_iter ? 1 : 0;
    }
    // the held-out rows, k3_simple's logistic arithmetic; class 1 iff dec > 0 (LinearClassifierMixin.predict)
    long long ok = 0;
    for (int64_t v = tid; v < J.n_va; v += BT) {
        const int64_t r = A.va_idx[J.va_off + v];
        const double *x = A.X + r * d;
        double dec = 0.0;
        for (int f = 0; f < d; ++f) dec += x[f] * s_w[f];
        dec += s_w[d];
        A.dec[J.va_off + v] = dec;
        ok += (dec > 0.0 ? 1 : 0) == A.y[r];
    }
    for (int o = 32; o > 0; o >>= 1) ok += __shfl_xor(ok, o);
    if (lane == 0) s_cnt[wave] = ok;
    __syncthreads();
    if (tid == 0) {
        long long c = 0;
        for (int w = 0; w < NWAVE; ++w) c += s_cnt[w];
        A.correct[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(BT) void k7_nb_fit(NbArgs A) {
    __shared__ double s_red[NWAVE][DMAX][3];
    __shared__ double s_theta[2][DMAX], s_var[2][DMAX], s_mu[DMAX], s_all[DMAX], s_cst[2];
    __shared__ long long s_cnt[NWAVE];

    const Job J = A.jobs[blockIdx.x];
    const int64_t l = J.n_tr, n0 = J.n_neg, n1 = l - n0;
    const int d = A.d, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t *tr = A.tr_idx + J.tr_off;
    auto x_at = [&](int64_t t, int f) { return A.X[(int64_t)tr[t] * d + f]; };

    // per feature three sums over the rows: classes_[0]'s rows (t < n0), classes_[1]'s, and all of them
    auto reduce3 = [&](auto &&term) {
        for (int f = 0; f < d; ++f) {
            double a = 0.0, b = 0.0, c = 0.0;
            for (int64_t t = tid; t < l; t += BT) {
                const double v = term(f, t);
                if (t < n0) a += v; else b += v;
                c += v;
            }
            a = wave_sum(a);
            b = wave_sum(b);
            c = wave_sum(c);
            if (lane == 0) { s_red[wave][f][0] = a; s_red[wave][f][1] = b; s_red[wave][f][2] = c; }
        }
        __syncthreads();
    };
    auto fold = [&](int f, int k) {
        double s = 0.0;
        for (int w = 0; w < NWAVE; ++w) s += s_red[w][f][k];
        return s;
    };

    reduce3([&](int f, int64_t t) { return x_at(t, f); });                 // the means
    if (tid < d) {
        s_theta[0][tid] = fold(tid, 0) / (double)n0;
        s_theta[1][tid] = fold(tid, 1) / (double)n1;
        s_mu[tid] = fold(tid, 2) / (double)l;
    }
    __syncthreads();
    reduce3([&](int f, int64_t t) {                                         // the centred sums of squares
        const double x = x_at(t, f), m = t < n0 ? s_theta[0][f] : s_theta[1][f];
        const double a = x - m;
        return a * a;
    });
    if (tid < d) {
        s_var[0][tid] = fold(tid, 0) / (double)n0;
        s_var[1][tid] = fold(tid, 1) / (double)n1;
    }
    __syncthreads();
    // (the job-wide variance needs the job-wide mean: its own pass)
    for (int f = 0; f < d; ++f) {
        double c = 0.0;
        for (int64_t t = tid; t < l; t += BT) {
            const double a = x_at(t, f) - s_mu[f];
            c += a * a;
        }
        c = wave_sum(c);
        if (lane == 0) s_red[wave][f][2] = c;
    }
    __syncthreads();
    if (tid < d) s_all[tid] = fold(tid, 2) / (double)l;
    __syncthreads();
    double eps = 0.0;
    for (int f = 0; f < d; ++f) eps = fmax(eps, s_all[f]);
    eps = A.var_smoothing * eps;
    __syncthreads();
    if (tid < d) {
        s_var[0][tid] += eps;
        s_var[1][tid] += eps;
    }
    __syncthreads();
    if (tid < 2) {                                                          // log prior - 0.5 sum log(2 pi var)
        const double *v = s_var[tid];
        const double prior = (double)(tid == 0 ? n0 : n1) / (double)(n0 + n1);
        s_cst[tid] = log(prior) + (-0.5 * np_sum(d, [&](int i) { return log(2.0 * 3.14159265358979323846 * v[i]); }));
    }
    __syncthreads();
    const int64_t job = blockIdx.x;
    if (tid < d) {
        for (int c = 0; c < 2; ++c) {
            A.theta[(job * 2 + c) * d + tid] = s_theta[c][tid];
            A.var[(job * 2 + c) * d + tid] = s_var[c][tid];
        }
    }
    if (tid == 0) A.epsilon[job] = eps;

    // the held-out rows: argmax of the joint log-likelihood, ties to class 0 (GaussianNB.predict), in k3_simple's arithmetic
    long long ok = 0;
    if (eps > 0.0) {
        for (int64_t v = tid; v < J.n_va; v += BT) {
            const int64_t r = A.va_idx[J.va_off + v];
            const double *x = A.X + r * d;
            double jll[2];
            for (int c = 0; c < 2; ++c) {
                const double *th = s_theta[c], *vr = s_var[c];
                jll[c] = s_cst[c] - 0.5 * np_sum(d, [&](int i) {
                    const double t = x[i] - th[i];
                    return (t * t) / vr[i];
                });
            }
            ok += (jll[1] > jll[0] ? 1 : 0) == A.y[r];
        }
    }
    for (int o = 32; o > 0; o >>= 1) ok += __shfl_xor(ok, o);
    if (lane == 0) s_cnt[wave] = ok;
    __syncthreads();
    if (tid == 0) {
        long long c = 0;
        for (int w = 0; w < NWAVE; ++w) c += s_cnt[w];
        A.correct[job] = c;
    }
}

// the checks both fits share, then the jobs with their rows grouped classes_[0] first (stable) -> 0, or -12 with the error set
int plan_jobs(const char *who, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in, int32_t n_jobs,
              const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx,
              std::vector<Job> &jobs, std::vector<int32_t> &grouped) {
    const int d = n_in;
    if (d < 1 || d > DMAX) { mc_set_error("%s: n_in %d out of range 1..%d", who, d, DMAX); return -12; }
    if (n_samples < 2 || n_samples > MAX_ROWS || n_jobs < 1 || n_jobs > 65535) {
        mc_set_error("%s: %lld samples, %d jobs out of range", who, (long long)n_samples, n_jobs);
        return -12;
    }
    std::vector<int64_t> n_neg((size_t)n_jobs);
    if (int rc = check_jobs(who, X, y, n_samples, d, n_jobs, train_off, train_idx, val_off, val_idx, MAX_ROWS, 2, true, false, n_neg.data()))
        return rc;
    jobs.resize((size_t)n_jobs);
    grouped.resize((size_t)train_off[n_jobs]);
    for (int j = 0; j < n_jobs; ++j) {
        jobs[j] = Job{train_off[j], train_off[j + 1] - train_off[j], n_neg[j], val_off[j], val_off[j + 1] - val_off[j], 0u, 0};
        int64_t a = train_off[j], b = train_off[j] + n_neg[j];
        for (int64_t i = train_off[j]; i < train_off[j + 1]; ++i) {
            const int32_t r = train_idx[i];
            grouped[(size_t)(y[r] == 0 ? a++ : b++)] = r;
        }
    }
    return 0;
}

}  // namespace

extern "C" int mc_lr_fit(mc_ctx *c, const mc_lr_params *P, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in,
                         int32_t n_jobs, const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off,
                         const int32_t *val_idx, const uint32_t *seeds, double *coef, double *intercept, int32_t *n_iter,
                         int32_t *status, int64_t *val_correct, double *val_dec) {
    if (!P || !X || !y || !train_off || !train_idx || !val_off || !seeds || !coef || !intercept || !n_iter || !status || !val_correct) {
        mc_set_error("mc_lr_fit: a required pointer is NULL");
        return -12;
    }
    if (!(P->C > 0.0) || !std::isfinite(P->C)) { mc_set_error("mc_lr_fit: C must be finite and > 0"); return -12; }
    if (!(P->tol > 0.0) || !std::isfinite(P->tol)) { mc_set_error("mc_lr_fit: tol must be finite and > 0"); return -12; }
    if (P->max_iter < 1 || P->max_iter > 1000000) { mc_set_error("mc_lr_fit: max_iter %d out of range 1..10^6", P->max_iter); return -12; }
    std::vector<Job> jobs;
    std::vector<int32_t> grouped;
    int rc = plan_jobs("mc_lr_fit", X, y, n_samples, n_in, n_jobs, train_off, train_idx, val_off, val_idx, jobs, grouped);
    if (rc) return rc;
    const int d = n_in, n = d + 1;
    const int64_t n_tr = train_off[n_jobs], n_va = val_off[n_jobs];
    if (n_va > 0 && !val_dec) { mc_set_error("mc_lr_fit: a required pointer is NULL"); return -12; }
    for (int j = 0; j < n_jobs; ++j) jobs[j].seed = seeds[j];
    const double bytes = ((double)n_tr * (n + 5) + (double)n_samples * d + (double)n_va) * 8.0 + (double)n_tr * 4 + (double)n_va * 4 +
                         (double)n_samples;
    if (bytes > (double)MEM_CAP) {
        mc_set_error("mc_lr_fit: %.0f bytes of work memory exceed the cap of %lld", bytes, (long long)MEM_CAP);
        return -12;
    }
    if ((rc = select_device("mc_lr_fit", c))) return rc;
    Pool pool("mc_lr_fit");
    double *dX = pool.get<double>((size_t)n_samples * d), *dXc = pool.get<double>((size_t)n_tr * n);
    uint8_t *dy = pool.get<uint8_t>((size_t)n_samples);
    int32_t *dtr = pool.get<int32_t>((size_t)n_tr), *dva = pool.get<int32_t>((size_t)n_va);
    Job *djobs = pool.get<Job>((size_t)n_jobs);
    double *rows = pool.get<double>((size_t)n_tr * 5);
    double *dw = pool.get<double>((size_t)n_jobs * n), *ddec = pool.get<double>((size_t)n_va);
    int *diter = pool.get<int>((size_t)n_jobs), *dstatus = pool.get<int>((size_t)n_jobs);
    long long *dcorrect = pool.get<long long>((size_t)n_jobs);
    if (!pool.ok) return -10;
    Xfer x("mc_lr_fit", mc_internal_stream(c));
    x.up(dX, X, (size_t)n_samples * d);
    x.up(dy, y, (size_t)n_samples);
    x.up(dtr, grouped.data(), grouped.size());
    x.up(dva, val_idx, (size_t)n_va);
    x.up(djobs, jobs.data(), jobs.size());
    x.launch(k7_lr_fit, dim3((unsigned)n_jobs), dim3(BT), 0,
             LrArgs{dX, dy, dtr, dva, djobs, dXc, rows, rows + n_tr, rows + 2 * n_tr, rows + 3 * n_tr, rows + 4 * n_tr,
                    d, P->max_iter, P->C, P->tol, dw, diter, dstatus, ddec, dcorrect});
    std::vector<double> hw((size_t)n_jobs * n);
    x.down(hw.data(), dw, hw.size());
    x.down(n_iter, diter, (size_t)n_jobs);
    x.down(status, dstatus, (size_t)n_jobs);
    x.down(val_correct, dcorrect, (size_t)n_jobs);
    x.down(val_dec, ddec, (size_t)n_va);
    x.sync();
    if (!x.ok()) return x.fail();
    for (int j = 0; j < n_jobs; ++j) {
        for (int f = 0; f < d; ++f) coef[(size_t)j * d + f] = hw[(size_t)j * n + f];
        intercept[j] = hw[(size_t)j * n + d];
    }
    return 0;
}

extern "C" int mc_nb_fit(mc_ctx *c, const mc_nb_params *P, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in,
                         int32_t n_jobs, const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off,
                         const int32_t *val_idx, double *theta, double *var, double *epsilon, int64_t *class_count,
                         int64_t *val_correct) {
    if (!P || !X || !y || !train_off || !train_idx || !val_off || !theta || !var || !epsilon || !class_count || !val_correct) {
        mc_set_error("mc_nb_fit: a required pointer is NULL");
        return -12;
    }
    if (!(P->var_smoothing > 0.0) || !std::isfinite(P->var_smoothing)) {
        mc_set_error("mc_nb_fit: var_smoothing must be finite and > 0");
        return -12;
    }
    std::vector<Job> jobs;
    std::vector<int32_t> grouped;
    int rc = plan_jobs("mc_nb_fit", X, y, n_samples, n_in, n_jobs, train_off, train_idx, val_off, val_idx, jobs, grouped);
    if (rc) return rc;
    const int d = n_in;
    const int64_t n_tr = train_off[n_jobs], n_va = val_off[n_jobs];
    const double bytes = ((double)n_samples * d + (double)n_jobs * (4 * d + 4)) * 8.0 + (double)(n_tr + n_va) * 4 + (double)n_samples;
    if (bytes > (double)MEM_CAP) {
        mc_set_error("mc_nb_fit: %.0f bytes of work memory exceed the cap of %lld", bytes, (long long)MEM_CAP);
        return -12;
    }
    if ((rc = select_device("mc_nb_fit", c))) return rc;
    Pool pool("mc_nb_fit");
    double *dX = pool.get<double>((size_t)n_samples * d);
    uint8_t *dy = pool.get<uint8_t>((size_t)n_samples);
    int32_t *dtr = pool.get<int32_t>((size_t)n_tr), *dva = pool.get<int32_t>((size_t)n_va);
    Job *djobs = pool.get<Job>((size_t)n_jobs);
    double *dtheta = pool.get<double>((size_t)n_jobs * 2 * d), *dvar = pool.get<double>((size_t)n_jobs * 2 * d);
    double *deps = pool.get<double>((size_t)n_jobs);
    long long *dcorrect = pool.get<long long>((size_t)n_jobs);
    if (!pool.ok) return -10;
    Xfer x("mc_nb_fit", mc_internal_stream(c));
    x.up(dX, X, (size_t)n_samples * d);
    x.up(dy, y, (size_t)n_samples);
    x.up(dtr, grouped.data(), grouped.size());
    x.up(dva, val_idx, (size_t)n_va);
    x.up(djobs, jobs.data(), jobs.size());
    x.launch(k7_nb_fit, dim3((unsigned)n_jobs), dim3(BT), 0, NbArgs{dX, dy, dtr, dva, djobs, d, P->var_smoothing, dtheta, dvar, deps, dcorrect});
    x.down(theta, dtheta, (size_t)n_jobs * 2 * d);
    x.down(var, dvar, (size_t)n_jobs * 2 * d);
    x.down(epsilon, deps, (size_t)n_jobs);
    x.down(val_correct, dcorrect, (size_t)n_jobs);
    x.sync();
    if (!x.ok()) return x.fail();
    for (int j = 0; j < n_jobs; ++j) {
        class_count[2 * j] = jobs[j].n_neg;
        class_count[2 * j + 1] = jobs[j].n_tr - jobs[j].n_neg;
    }
    for (int j = 0; j < n_jobs; ++j)
        if (!(epsilon[j] > 0.0)) {
            mc_set_error("mc_nb_fit: job %d's training rows are all equal (epsilon_ = 0: every variance is 0)", j);
            return -12;
        }
    return 0;
}
