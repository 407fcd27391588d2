// libmcaller_hip.so -- the RBF support-vector fit behind `--train -c SVM` on the GPU (gfx950 / MI355X).  C ABI: include/mcaller_hip.h.
//
// The reference fits SVC(kernel='rbf', probability=True) per sub-model, five times for GroupKFold and once more on all rows
// (train_model.py:51-53,:62-65,:92-101); the final fit's Platt scaling adds five more solves (libsvm's svm_binary_svc_probability).
// Every solve is one workgroup of k6_svm_fit; no workgroup waits for another.  The algorithm is libsvm's Solver without shrinking
// (tests/svm_fit_oracle.py restates it in NumPy):
//
//   * G = -1, alpha = 0.  Each iteration picks i = argmax -y_t G_t over I_up (a block argmax), computes kernel row i and picks j by
//     libsvm's second-order rule over I_low (a block argmin; the same pass takes Gmax2), stops when Gmax + Gmax2 < eps, updates the
//     pair with libsvm's two clipping cases and, in the pass that computes kernel row j, G and the next i.  Ties go to the lowest
//     index.  At most max(10^7, 100 l) iterations (status 1 past that, scikit-learn's fit_status_ = 1).
//   * rho is the mean of y G over the free alphas, or the midpoint of the bounds when there are none.
//   * Kernel values in fp64 in the difference form, exp(-gamma sum_f (x_f - x'_f)^2), f in order: exact 1 at x = x'.
//   * A lane owns the rows t = tid + BT r: alpha, G and the kernel row i live in global memory (L2-resident at these sizes) and only
//     the owner reads or writes its rows, so the block reductions are the only barriers (two per iteration, LDS double-buffered).
// k6_svm_val then scores each job's held-out rows as k3_svm does (support vectors in order, dec += coef exp(-gamma d2), + intercept),
// the sign turned so that dec > 0 means classes_[0]; k6_svm_sigmoid is libsvm's sigmoid_train in one workgroup, fixed-order sums.
// The entry points' allocations, transfers and job checks, FitJob, splitmix64 and wave_sum: mc_fit.h.
#include <cstdlib>

#include "mc_fit.h"

namespace {

constexpr int BT = 1024;                        // threads per solve
constexpr int NWAVE = BT / 64;
constexpr int DMAX = 64;                        // features
constexpr double TAU = 1e-12;
constexpr int64_t MAX_ROWS = (int64_t)1 << 26;  // per job and per call
constexpr int64_t MEM_CAP = (int64_t)4 << 30;   // device work memory of one call, bytes

struct SJob {
    int64_t tr_off, n_tr, va_off, n_va;
    double gamma;
    int64_t max_iter;
    int32_t sign;                               // +1: the job's +1 rows are classes_[0] (its first row's class), else -1
    int32_t pad;
};

struct FitArgs {
    const double *Xt;                           // per job [d][n_tr], at tr_off * d
    const int8_t *ys;                           // solve labels +1 / -1, at tr_off
    const SJob *jobs;
    double *alpha, *G, *Ki;                     // at tr_off
    double *rho;
    long long *n_iter;
    int *status;
    int d;
    double C, eps;
};

struct ValArgs {
    const double *X;                            // [n][d]
    const uint8_t *y;
    const int32_t *va_idx;
    const double *Xt;
    const int8_t *ys;
    const double *alpha, *rho;
    const SJob *jobs;
    int d;
    double *dec;                                // at va_off
    unsigned long long *correct;
};

__device__ __forceinline__ double kval(const double *Xt, int64_t l, int d, int64_t a, int64_t b, double gamma) {
    double d2 = 0.0;
    for (int f = 0; f < d; ++f) {
        const double t = Xt[f * l + a] - Xt[f * l + b];
        d2 += t * t;
    }
    return exp(-gamma * d2);
}

__global__ __launch_bounds__(BT) void k6_svm_fit(FitArgs A) {
    __shared__ double s_v[2][NWAVE], s_p[2][NWAVE][3], s_g[NWAVE], s_u[NWAVE];
    __shared__ int s_i[2][NWAVE], s_n[NWAVE];
    const SJob J = A.jobs[blockIdx.x];
    const int64_t l = J.n_tr;
    const int d = A.d, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *Xt = A.Xt + J.tr_off * d;
    const int8_t *ys = A.ys + J.tr_off;
    double *alpha = A.alpha + J.tr_off, *G = A.G + J.tr_off, *Ki = A.Ki + J.tr_off;
    const double C = A.C, eps = A.eps, gamma = J.gamma;

    // a block argmax (buffer b) carrying the winner's row values p[3] (a lane reads and writes only its own rows in global memory,
    // so what every lane needs of rows i and j travels here); every lane leaves with the same (v, i, p)
    auto argmax = [&](double &v, int &ix, double *p, int b) {
        for (int o = 32; o > 0; o >>= 1) {
            const double v2 = __shfl_xor(v, o);
            const int i2 = __shfl_xor(ix, o);
            double q[3];
            for (int c = 0; c < 3; ++c) q[c] = __shfl_xor(p[c], o);
            if (i2 >= 0 && (ix < 0 || v2 > v || (v2 == v && i2 < ix))) {
                v = v2; ix = i2;
                for (int c = 0; c < 3; ++c) p[c] = q[c];
            }
        }
        if (lane == 0) {
            s_v[b][wave] = v; s_i[b][wave] = ix;
            for (int c = 0; c < 3; ++c) s_p[b][wave][c] = p[c];
        }
        __syncthreads();
        v = -INFINITY; ix = -1;
        for (int w = 0; w < NWAVE; ++w) {
            const double v2 = s_v[b][w];
            const int i2 = s_i[b][w];
            if (i2 >= 0 && (ix < 0 || v2 > v || (v2 == v && i2 < ix))) {
                v = v2; ix = i2;
                for (int c = 0; c < 3; ++c) p[c] = s_p[b][w][c];
            }
        }
    };
    // I_up: y = +1 below C, y = -1 above 0; the candidate's value -y G, its payload (alpha, G)
    auto up_candidate = [&](int64_t t, double a, double g, double &v, int &ix, double *p) {
        const int yt = ys[t];
        if (yt > 0 ? a < C : a > 0.0) {
            const double c = -(double)yt * g;
            if (ix < 0 || c > v) { v = c; ix = (int)t; p[0] = a; p[1] = g; }   // (t rises: the first of equals stays)
        }
    };

    double v = -INFINITY, pi[3] = {0.0, 0.0, 0.0};
    int i = -1;
    for (int64_t t = tid; t < l; t += BT) {
        alpha[t] = 0.0;
        G[t] = -1.0;
        up_candidate(t, 0.0, -1.0, v, i, pi);
    }
    argmax(v, i, pi, 0);
    double Gmax = v;
    int64_t iter = 0;
    int status = 0;
    for (;;) {
        if (iter >= J.max_iter) { status = 1; break; }
        if (i < 0) break;
        // kernel row i; j by the second-order rule over I_low (payload alpha_j, G_j, K_ij); Gmax2
        const int yi = ys[i];
        double jv = -INFINITY, gmax2 = -INFINITY, pj[3] = {0.0, 0.0, 0.0};
        int j = -1;
        for (int64_t t = tid; t < l; t += BT) {
            const double k = kval(Xt, l, d, i, t, gamma);
            Ki[t] = k;
            const int yt = ys[t];
            const double a = alpha[t], g = G[t];
            if (yt > 0 ? a > 0.0 : a < C) {
                const double yg = yt > 0 ? g : -g;
                gmax2 = fmax(gmax2, yg);
                const double grad_diff = Gmax + yg;
                if (grad_diff > 0.0) {
                    const double quad = 1.0 + 1.0 - 2.0 * k;
                    const double obj = -(grad_diff * grad_diff) / (quad > 0.0 ? quad : TAU);
                    if (j < 0 || -obj > jv) { jv = -obj; j = (int)t; pj[0] = a; pj[1] = g; pj[2] = k; }
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) gmax2 = fmax(gmax2, __shfl_xor(gmax2, o));
        if (lane == 0) s_g[wave] = gmax2;
        argmax(jv, j, pj, 1);                   // (its barrier publishes s_g too)
        gmax2 = -INFINITY;
        for (int w = 0; w < NWAVE; ++w) gmax2 = fmax(gmax2, s_g[w]);
        if (Gmax + gmax2 < eps || j < 0) break;
        ++iter;

        // the pair update, the same arithmetic in every lane (libsvm's two cases, C_i = C_j = C, QD = 1)
        const int yj = ys[j];
        const double ai0 = pi[0], aj0 = pj[0], Gi = pi[1], Gj = pj[1], Qij = (double)(yi * yj) * pj[2];
        double ai = ai0, aj = aj0;
        if (yi != yj) {
            double quad = 1.0 + 1.0 + 2.0 * Qij;
            if (quad <= 0.0) quad = TAU;
            const double delta = (-Gi - Gj) / quad, diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
            if (diff > C - C) { if (ai > C) { ai = C; aj = C - diff; } }
            else { if (aj > C) { aj = C; ai = C + diff; } }
        } else {
            double quad = 1.0 + 1.0 - 2.0 * Qij;
            if (quad <= 0.0) quad = TAU;
            const double delta = (Gi - Gj) / quad, sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > C) { if (ai > C) { ai = C; aj = sum - C; } }
            else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
            if (sum > C) { if (aj > C) { aj = C; ai = sum - C; } }
            else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
        }
        const double dai = ai - ai0, daj = aj - aj0;
        // kernel row j, G, the owners' alphas and the next i
        v = -INFINITY;
        int ni = -1;
        for (int64_t t = tid; t < l; t += BT) {
            const int yt = ys[t];
            const double qi = (double)(yi * yt) * Ki[t], qj = (double)(yj * yt) * kval(Xt, l, d, j, t, gamma);
            const double g = G[t] + (qi * dai + qj * daj);
            G[t] = g;
            double a = alpha[t];
            if (t == i) { a = ai; alpha[t] = a; }
            if (t == j) { a = aj; alpha[t] = a; }
            up_candidate(t, a, g, v, ni, pi);
        }
        argmax(v, ni, pi, 0);
        Gmax = v;
        i = ni;
    }

    // rho: the mean of y G over the free alphas, or the midpoint of the bounds
    double ub = INFINITY, lb = -INFINITY, sum = 0.0;
    int nfree = 0;
    for (int64_t t = tid; t < l; t += BT) {
        const int yt = ys[t];
        const double a = alpha[t], yg = (double)yt * G[t];
        if (a >= C) { if (yt < 0) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
        else if (a <= 0.0) { if (yt > 0) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
        else { ++nfree; sum += yg; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ub = fmin(ub, __shfl_xor(ub, o));
        lb = fmax(lb, __shfl_xor(lb, o));
        sum += __shfl_xor(sum, o);
        nfree += __shfl_xor(nfree, o);
    }
    __syncthreads();                            // (s_v[1] was read after the last barrier)
    if (lane == 0) { s_v[1][wave] = ub; s_g[wave] = lb; s_u[wave] = sum; s_n[wave] = nfree; }
    __syncthreads();
    if (tid == 0) {
        ub = INFINITY; lb = -INFINITY; sum = 0.0; nfree = 0;
        for (int w = 0; w < NWAVE; ++w) {
            ub = fmin(ub, s_v[1][w]);
            lb = fmax(lb, s_g[w]);
            sum += s_u[w];
            nfree += s_n[w];
        }
        A.rho[blockIdx.x] = nfree > 0 ? sum / nfree : (ub + lb) / 2;
        A.n_iter[blockIdx.x] = (long long)iter;
        A.status[blockIdx.x] = status;
    }
}

// a lane per held-out row: libsvm's decision value in k3_svm's arithmetic, turned to "dec > 0: classes_[0]"
__global__ __launch_bounds__(256) void k6_svm_val(ValArgs V) {
    const int job = blockIdx.y;
    const SJob J = V.jobs[job];
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (v < J.n_va) {
        const int d = V.d;
        const int64_t r = V.va_idx[J.va_off + v], l = J.n_tr;
        const double *Xt = V.Xt + J.tr_off * d, *alpha = V.alpha + J.tr_off;
        const int8_t *ys = V.ys + J.tr_off;
        const double *x = V.X + r * d;
        double dec = 0.0;
        for (int64_t t = 0; t < l; ++t) {
            const double a = alpha[t];
            if (!(a > 0.0)) continue;
            double d2 = 0.0;
            for (int f = 0; f < d; ++f) {
                const double q = x[f] - Xt[f * l + t];
                d2 += q * q;
            }
            dec += (ys[t] > 0 ? a : -a) * exp(-J.gamma * d2);
        }
        dec = dec + (-V.rho[job]);
        if (J.sign < 0) dec = -dec;
        V.dec[J.va_off + v] = dec;
        ok = (dec > 0.0 ? 0 : 1) == V.y[r];
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&V.correct[job], (unsigned long long)__popcll(m));
}

// libsvm's sigmoid_train (Platt scaling with Lin et al.'s Newton steps) in one workgroup: every sum is a lane's rows in order, then
// the lanes of a wave by a butterfly, then the waves in order -- the same bits on every run
constexpr int ST = 1024, SWAVE = ST / 64;

__global__ __launch_bounds__(ST) void k6_svm_sigmoid(const double *__restrict__ dec, const uint8_t *__restrict__ y, int64_t n,
                                                     double *__restrict__ out) {
    __shared__ double s_r[2][SWAVE][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int buf = 0;
    auto reduce = [&](double *s, int m) {       // s[0..m): this lane's partial sums -> the block's
        for (int o = 32; o > 0; o >>= 1)
            for (int c = 0; c < m; ++c) s[c] += __shfl_xor(s[c], o);
        if (lane == 0)
            for (int c = 0; c < m; ++c) s_r[buf][wave][c] = s[c];
        __syncthreads();
        for (int c = 0; c < m; ++c) {
            double a = 0.0;
            for (int w = 0; w < SWAVE; ++w) a += s_r[buf][w][c];
            s[c] = a;
        }
        buf ^= 1;
    };
    double s[5];
    s[0] = 0.0;
    for (int64_t k = tid; k < n; k += ST) s[0] += y[k] == 0 ? 1.0 : 0.0;
    reduce(s, 1);
    const double prior1 = s[0], prior0 = (double)n - prior1;
    const double hiTarget = (prior1 + 1.0) / (prior1 + 2.0), loTarget = 1 / (prior0 + 2.0);
    const double min_step = 1e-10, sigma = 1e-12, eps = 1e-5;
    auto fsum = [&](double A, double B) {
        double f[1] = {0.0};
        for (int64_t k = tid; k < n; k += ST) {
            const double t = y[k] == 0 ? hiTarget : loTarget, fApB = dec[k] * A + B;
            if (fApB >= 0) f[0] += t * fApB + log(1 + exp(-fApB));
            else f[0] += (t - 1) * fApB + log(1 + exp(fApB));
        }
        reduce(f, 1);
        return f[0];
    };
    double A = 0.0, B = log((prior0 + 1.0) / (prior1 + 1.0));
    double fval = fsum(A, B);
    for (int iter = 0; iter < 100; ++iter) {
        for (int c = 0; c < 5; ++c) s[c] = 0.0;             // h11, h22, h21, g1, g2 (sigma added after the sum)
        for (int64_t k = tid; k < n; k += ST) {
            const double t = y[k] == 0 ? hiTarget : loTarget, dv = dec[k], fApB = dv * A + B;
            double p, q;
            if (fApB >= 0) { p = exp(-fApB) / (1.0 + exp(-fApB)); q = 1.0 / (1.0 + exp(-fApB)); }
            else { p = 1.0 / (1.0 + exp(fApB)); q = exp(fApB) / (1.0 + exp(fApB)); }
            const double d2 = p * q, d1 = t - p;
            s[0] += dv * dv * d2;
            s[1] += d2;
            s[2] += dv * d2;
            s[3] += dv * d1;
            s[4] += d1;
        }
        reduce(s, 5);
        const double h11 = sigma + s[0], h22 = sigma + s[1], h21 = s[2], g1 = s[3], g2 = s[4];
        if (fabs(g1) < eps && fabs(g2) < eps) break;
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double stepsize = 1;
        while (stepsize >= min_step) {                      // (at most 34 halvings)
            const double newA = A + stepsize * dA, newB = B + stepsize * dB;
            const double newf = fsum(newA, newB);
            if (newf < fval + 0.0001 * stepsize * gd) { A = newA; B = newB; fval = newf; break; }
            stepsize = stepsize / 2.0;
        }
        if (stepsize < min_step) break;
    }
    if (tid == 0) { out[0] = A; out[1] = B; }
}

}  // namespace

extern "C" int mc_svm_fit(mc_ctx *c, const mc_svm_params *P, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in,
                          int32_t n_jobs, const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off,
                          const int32_t *val_idx, const double *gamma, double *alpha, double *rho, int64_t *n_iter, int32_t *status,
                          int64_t *val_correct, double *val_dec) {
    if (!P || !X || !y || !train_off || !train_idx || !val_off || !gamma || !alpha || !rho || !n_iter || !status || !val_correct) {
        mc_set_error("mc_svm_fit: a required pointer is NULL");
        return -12;
    }
    const int d = n_in;
    if (d < 1 || d > DMAX) { mc_set_error("mc_svm_fit: n_in %d out of range 1..%d", d, DMAX); return -12; }
    if (!(P->C > 0.0) || !std::isfinite(P->C)) { mc_set_error("mc_svm_fit: C must be finite and > 0"); return -12; }
    if (!(P->tol > 0.0) || !std::isfinite(P->tol)) { mc_set_error("mc_svm_fit: tol must be finite and > 0"); return -12; }
    if (P->max_iter < 0) { mc_set_error("mc_svm_fit: max_iter %lld < 0", (long long)P->max_iter); return -12; }
    if (n_samples < 2 || n_samples > MAX_ROWS || n_jobs < 1 || n_jobs > 65535) {
        mc_set_error("mc_svm_fit: %lld samples, %d jobs out of range", (long long)n_samples, n_jobs);
        return -12;
    }
    if (int rc = check_jobs("mc_svm_fit", X, y, n_samples, d, n_jobs, train_off, train_idx, val_off, val_idx, MAX_ROWS, 2, true, false, nullptr))
        return rc;
    int64_t max_va = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!(gamma[j] > 0.0) || !std::isfinite(gamma[j])) { mc_set_error("mc_svm_fit: gamma of job %d must be finite and > 0", j); return -12; }
        max_va = std::max(max_va, val_off[j + 1] - val_off[j]);
    }
    const int64_t n_tr = train_off[n_jobs], n_va = val_off[n_jobs];
    if (n_va > 0 && !val_dec) { mc_set_error("mc_svm_fit: a required pointer is NULL"); return -12; }
    const double bytes = ((double)n_tr * (d + 3) + (double)n_samples * d + (double)n_va) * 8.0 + (double)n_tr + (double)n_samples;
    if (bytes > (double)MEM_CAP) {
        mc_set_error("mc_svm_fit: %.0f bytes of work memory exceed the cap of %lld", bytes, (long long)MEM_CAP);
        return -12;
    }
    if (int rc = select_device("mc_svm_fit", c)) return rc;

    // host: each job's rows gathered feature-major, the solve labels (+1: the class of the job's first row, as libsvm's label[0])
    std::vector<double> Xt((size_t)n_tr * d);
    std::vector<int8_t> ys((size_t)n_tr);
    std::vector<SJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t o = train_off[j], l = train_off[j + 1] - o;
        const uint8_t first = y[train_idx[o]];
        for (int64_t t = 0; t < l; ++t) {
            const int64_t r = train_idx[o + t];
            ys[o + t] = y[r] == first ? 1 : -1;
            for (int f = 0; f < d; ++f) Xt[(size_t)(o * d + f * l + t)] = X[r * d + f];
        }
        jobs[j] = SJob{o, l, val_off[j], val_off[j + 1] - val_off[j], gamma[j],
                       P->max_iter > 0 ? P->max_iter : std::max<int64_t>(10000000, 100 * l), first == 0 ? 1 : -1, 0};
    }
    Pool pool("mc_svm_fit");
    double *dXt = pool.get<double>((size_t)n_tr * d), *dX = pool.get<double>((size_t)n_samples * d);
    int8_t *dys = pool.get<int8_t>((size_t)n_tr);
    uint8_t *dy = pool.get<uint8_t>((size_t)n_samples);
    SJob *djobs = pool.get<SJob>((size_t)n_jobs);
    double *dalpha = pool.get<double>((size_t)n_tr), *dG = pool.get<double>((size_t)n_tr), *dKi = pool.get<double>((size_t)n_tr);
    double *drho = pool.get<double>((size_t)n_jobs);
    long long *diter = pool.get<long long>((size_t)n_jobs);
    int *dstatus = pool.get<int>((size_t)n_jobs);
    int32_t *dva = pool.get<int32_t>((size_t)n_va);
    double *ddec = pool.get<double>((size_t)n_va);
    unsigned long long *dcorrect = pool.get<unsigned long long>((size_t)n_jobs);
    if (!pool.ok) return -10;
    Xfer x("mc_svm_fit", mc_internal_stream(c));
    x.up(dXt, Xt.data(), Xt.size());
    x.up(dX, X, (size_t)n_samples * d);
    x.up(dys, ys.data(), ys.size());
    x.up(dy, y, (size_t)n_samples);
    x.up(djobs, jobs.data(), jobs.size());
    x.up(dva, val_idx, (size_t)n_va);
    x.zero(dcorrect, (size_t)n_jobs);
    x.launch(k6_svm_fit, dim3((unsigned)n_jobs), dim3(BT), 0, FitArgs{dXt, dys, djobs, dalpha, dG, dKi, drho, diter, dstatus, d, P->C, P->tol});
    if (max_va > 0)
        x.launch(k6_svm_val, dim3((unsigned)((max_va + 255) / 256), (unsigned)n_jobs), dim3(256), 0,
                 ValArgs{dX, dy, dva, dXt, dys, dalpha, drho, djobs, d, ddec, dcorrect});
    std::vector<long long> hiter((size_t)n_jobs);
    std::vector<int> hstatus((size_t)n_jobs);
    x.down(alpha, dalpha, (size_t)n_tr);
    x.down(rho, drho, (size_t)n_jobs);
    x.down(hiter.data(), diter, (size_t)n_jobs);
    x.down(hstatus.data(), dstatus, (size_t)n_jobs);
    x.down(val_correct, dcorrect, (size_t)n_jobs);
    x.down(val_dec, ddec, (size_t)n_va);
    x.sync();
    if (!x.ok()) return x.fail();
    for (int j = 0; j < n_jobs; ++j) {
        n_iter[j] = hiter[j];
        status[j] = hstatus[j];
    }
    return 0;
}

extern "C" int mc_svm_sigmoid_train(mc_ctx *c, const double *dec, const uint8_t *y, int64_t n, double *A, double *B) {
    if (!dec || !y || !A || !B) { mc_set_error("mc_svm_sigmoid_train: a required pointer is NULL"); return -12; }
    if (n < 1 || n > MAX_ROWS) { mc_set_error("mc_svm_sigmoid_train: %lld values out of range 1..%lld", (long long)n, (long long)MAX_ROWS); return -12; }
    for (int64_t i = 0; i < n; ++i) {
        if (y[i] > 1) { mc_set_error("mc_svm_sigmoid_train: labels must be 0 or 1"); return -12; }
        if (!std::isfinite(dec[i])) { mc_set_error("mc_svm_sigmoid_train: a decision value is not finite"); return -12; }
    }
    if (int rc = select_device("mc_svm_sigmoid_train", c)) return rc;
    Pool pool("mc_svm_sigmoid_train");
    double *ddec = pool.get<double>((size_t)n), *dout = pool.get<double>(2);
    uint8_t *dy = pool.get<uint8_t>((size_t)n);
    if (!pool.ok) return -10;
    double out[2] = {0.0, 0.0};
    Xfer x("mc_svm_sigmoid_train", mc_internal_stream(c));
    x.up(ddec, dec, (size_t)n);
    x.up(dy, y, (size_t)n);
    x.launch(k6_svm_sigmoid, dim3(1), dim3(ST), 0, (const double *)ddec, (const uint8_t *)dy, n, dout);
    x.down(out, dout, 2);
    x.sync();
    if (!x.ok()) return x.fail();
    *A = out[0];
    *B = out[1];
    return 0;
}
