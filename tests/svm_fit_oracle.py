"""CPU restatement (numpy) of the `--train -c SVM` fit (mc_svm_fit, k6_svm_fit): what scikit-learn's SVC(kernel='rbf',
probability=True) computes through libsvm, as train_model.fit_svm_on_gpu splits it into solves.  TEST INFRASTRUCTURE: the yardstick
the device is held to, never the product.

* gamma='scale': 1 / (d X.var()) on the rows a fit is given (1.0 if the variance is 0), as SVC.fit resolves it.
* The solve: libsvm's Solver without shrinking -- G = -1, alpha = 0; i = argmax -y G over I_up, j by the second-order rule over
  I_low (tau = 1e-12), stop when Gmax + Gmax2 < eps; libsvm's two clipping cases; rho the mean of y G over the free alphas or the
  midpoint of the bounds.  Ties go to the lowest index.  Kernel values in fp64, exp(-gamma sum_f (x_f - x'_f)^2), f in order.
* Platt scaling (svm_binary_svc_probability): the rows grouped by class (classes_[0] first, label +1), shuffled with
  perm[i] <-> perm[i + bounded_rand_int(l - i)] (std::mt19937 and Lemire's bounded draw, scikit-learn's newrand.h), five folds of
  positions, a solve on each fold's complement (or dec = +-1 when it holds one class), then sigmoid_train in sequential Python floats.
"""
import math

import numpy as np

from tests import svm_oracle

TAU = 1e-12


def gamma_of(X):
    X = np.asarray(X, dtype=np.float64)
    var = X.var()
    return 1.0 / (X.shape[1] * var) if var != 0 else 1.0


def permutation(l, seed):
    """libsvm's shuffle, one draw at a time."""
    mt = np.random.MT19937()
    mt._legacy_seeding(int(seed))
    perm = list(range(l))
    for i in range(l):
        rng = l - i
        x = int(mt.random_raw())
        m = x * rng
        if (m & 0xFFFFFFFF) < rng:
            t = (-rng) & 0xFFFFFFFF
            if t >= rng:
                t -= rng
                if t >= rng:
                    t %= rng
            while (m & 0xFFFFFFFF) < t:
                x = int(mt.random_raw())
                m = x * rng
        j = i + (m >> 32)
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm, dtype=np.int64)


def kernel_rows(A, B, gamma):
    """K[a, b] = exp(-gamma sum_f (A[a, f] - B[b, f])^2), the differences squared and added feature by feature."""
    d2 = np.zeros((len(A), len(B)))
    for f in range(A.shape[1]):
        t = A[:, f][:, None] - B[:, f][None, :]
        d2 = d2 + t * t
    return np.exp(-gamma * d2)


def smo(X, ys, gamma, C=1.0, eps=1e-3, max_iter=None):
    """One solve on the rows X (in solve order) with labels ys in {+1, -1}.  -> dict(alpha, rho, n_iter, status)."""
    X = np.asarray(X, dtype=np.float64)
    ys = np.asarray(ys, dtype=np.float64)
    l = len(ys)
    if max_iter is None:
        max_iter = max(10 ** 7, 100 * l)
    cols = [np.ascontiguousarray(X[:, f]) for f in range(X.shape[1])]

    def row(i):
        d2 = np.zeros(l)
        for c in cols:
            t = c[i] - c
            d2 = d2 + t * t
        return np.exp(-gamma * d2)

    alpha = np.zeros(l)
    G = -np.ones(l)
    it, status = 0, 0
    pos = ys > 0
    while True:
        if it >= max_iter:
            status = 1
            break
        up = np.where(pos, alpha < C, alpha > 0)
        if not up.any():
            break
        v = np.where(up, -ys * G, -np.inf)
        i = int(np.argmax(v))                                 # (the first of equals)
        Gmax = v[i]
        Ki = row(i)
        low = np.where(pos, alpha > 0, alpha < C)
        yg = ys * G
        Gmax2 = yg[low].max() if low.any() else -np.inf
        gd = Gmax + yg
        cand = low & (gd > 0)
        quad = 1.0 + 1.0 - 2.0 * Ki
        obj = -(gd * gd) / np.where(quad > 0, quad, TAU)
        if Gmax + Gmax2 < eps or not cand.any():
            break
        j = int(np.argmax(np.where(cand, -obj, -np.inf)))
        it += 1
        yi, yj = ys[i], ys[j]
        ai0, aj0, Gi, Gj = alpha[i], alpha[j], G[i], G[j]
        Qij = (yi * yj) * Ki[j]
        ai, aj = ai0, aj0
        if yi != yj:
            q = 1.0 + 1.0 + 2.0 * Qij
            q = q if q > 0 else TAU
            delta = (-Gi - Gj) / q
            diff = ai - aj
            ai += delta
            aj += delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > C - C:
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
        else:
            q = 1.0 + 1.0 - 2.0 * Qij
            q = q if q > 0 else TAU
            delta = (Gi - Gj) / q
            s = ai + aj
            ai -= delta
            aj += delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
            elif aj < 0:
                aj, ai = 0.0, s
            if s > C:
                if aj > C:
                    aj, ai = C, s - C
            elif ai < 0:
                ai, aj = 0.0, s
        dai, daj = ai - ai0, aj - aj0
        Kj = row(j)
        G = G + (((yi * ys) * Ki) * dai + ((yj * ys) * Kj) * daj)
        alpha[i], alpha[j] = ai, aj
    return dict(alpha=alpha, rho=rho_of(alpha, ys, G, C), n_iter=it, status=status)


def rho_of(alpha, ys, G, C=1.0):
    yG = ys * G
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        return float(yG[free].mean())
    ub = np.concatenate([yG[upper & (ys < 0)], yG[lower & (ys > 0)], [np.inf]]).min()
    lb = np.concatenate([yG[upper & (ys > 0)], yG[lower & (ys < 0)], [-np.inf]]).max()
    return float((ub + lb) / 2)


def gradient(X, ys, alpha, gamma, chunk=2048):
    """G = Q alpha - 1 recomputed from alpha (Q_ts = y_t y_s K_ts)."""
    X = np.asarray(X, dtype=np.float64)
    sv = alpha > 0
    c = (ys * alpha)[sv]
    G = np.empty(len(ys))
    for a in range(0, len(ys), chunk):
        G[a:a + chunk] = ys[a:a + chunk] * (kernel_rows(X[a:a + chunk], X[sv], gamma) @ c) - 1.0
    return G


def kkt_violation(X, ys, alpha, gamma, C=1.0):
    """Gmax + Gmax2 of a solution, G recomputed: libsvm stops below eps."""
    G = gradient(X, ys, alpha, gamma)
    pos = ys > 0
    up = np.where(pos, alpha < C, alpha > 0)
    low = np.where(pos, alpha > 0, alpha < C)
    gmax = (-ys * G)[up].max() if up.any() else -np.inf
    gmax2 = (ys * G)[low].max() if low.any() else -np.inf
    return max(0.0, float(gmax + gmax2))


def dual_objective(X, coef, gamma, chunk=2048):
    """0.5 c^T K c - sum |c| over the support vectors X with dual coefficients c = y alpha."""
    X = np.asarray(X, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64).reshape(-1)
    q = 0.0
    for a in range(0, len(c), chunk):
        q += float(c[a:a + chunk] @ (kernel_rows(X[a:a + chunk], X, gamma) @ c))
    return 0.5 * q - float(np.abs(c).sum())


def sigmoid_train(dec, labels):
    """libsvm's sigmoid_train, sequential Python floats.  labels: +1 / -1 (> 0 counts as prior1).  -> (A, B)."""
    dec = [float(v) for v in dec]
    lab = [float(v) for v in labels]
    l = len(dec)
    prior1 = float(sum(1 for v in lab if v > 0))
    prior0 = float(l) - prior1
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hiTarget = (prior1 + 1.0) / (prior1 + 2.0)
    loTarget = 1 / (prior0 + 2.0)
    t = [hiTarget if v > 0 else loTarget for v in lab]
    A, B = 0.0, math.log((prior0 + 1.0) / (prior1 + 1.0))

    def fun(A, B):
        f = 0.0
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                f += t[i] * fApB + math.log(1 + math.exp(-fApB))
            else:
                f += (t[i] - 1) * fApB + math.log(1 + math.exp(fApB))
        return f

    fval = fun(A, B)
    for _ in range(max_iter):
        h11, h22, h21, g1, g2 = sigma, sigma, 0.0, 0.0, 0.0
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                p = math.exp(-fApB) / (1.0 + math.exp(-fApB))
                q = 1.0 / (1.0 + math.exp(-fApB))
            else:
                p = 1.0 / (1.0 + math.exp(fApB))
                q = math.exp(fApB) / (1.0 + math.exp(fApB))
            d2 = p * q
            h11 += dec[i] * dec[i] * d2
            h22 += d2
            h21 += dec[i] * d2
            d1 = t[i] - p
            g1 += dec[i] * d1
            g2 += d1
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        stepsize = 1
        while stepsize >= min_step:
            newA, newB = A + stepsize * dA, B + stepsize * dB
            newf = fun(newA, newB)
            if newf < fval + 0.0001 * stepsize * gd:
                A, B, fval = newA, newB, newf
                break
            stepsize = stepsize / 2.0
        if stepsize < min_step:
            break
    return A, B


def grouped(rows, y, first):
    rows = np.asarray(rows)
    return np.concatenate([rows[y[rows] == first], rows[y[rows] != first]])


def solve_job(X, y, train, val, gamma):
    """A solve on rows `train` (solve order: the first row's class is +1) and the decision values of rows `val`, turned so that
    > 0 means class 0.  -> dict(alpha, rho, n_iter, status, val_dec, val_correct)."""
    ys = np.where(y[train] == y[train[0]], 1.0, -1.0)
    s = smo(X[train], ys, gamma)
    sign = 1.0 if y[train[0]] == 0 else -1.0
    sv = s['alpha'] > 0
    dec = sign * svm_oracle.decision(X[train][sv], (ys * s['alpha'])[sv], gamma, -s['rho'], X[val]) if len(val) else np.zeros(0)
    s.update(val_dec=dec, val_correct=int((np.where(dec > 0, 0, 1) == y[val]).sum()))
    return s


def platt_seed(seed):
    return int(seed % (2 ** 31 - 1))


def fit_submodel(X, y, jobs, seed):
    """The whole -c SVM fit of a sub-model: jobs = train_model.cv_jobs' six (train, val) jobs, seed = the final job's seed.
    -> dict(cv=[solve of fold f or None], gammas, final (solve), order, perm, platt_dec, A, B, fit: as train_model.fit_svm_on_gpu's)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y)
    cv, gammas = [], []
    for tr, va in jobs[:5]:
        g = gamma_of(X[tr])
        gammas.append(g)
        cv.append(solve_job(X, y, grouped(tr, y, 0), va, g) if len(set(y[tr].tolist())) == 2 else None)
    order = grouped(np.arange(len(y)), y, 0)
    gamma = gamma_of(X)
    final = solve_job(X, y, order, np.zeros(0, dtype=np.int64), gamma)
    l = len(order)
    perm = permutation(l, platt_seed(seed))
    dec = np.zeros(l)
    platt = []
    for f in range(5):
        begin, end = f * l // 5, (f + 1) * l // 5
        comp = order[np.concatenate([perm[:begin], perm[end:]])]
        held = perm[begin:end]
        labs = set(y[comp].tolist())
        if len(labs) == 2:
            s = solve_job(X, y, grouped(comp, y, 1), order[held], gamma)
            dec[held] = s['val_dec']
            platt.append(s)
        else:
            dec[held] = 0.0 if not labs else (1.0 if labs == {0} else -1.0)
            platt.append(None)
    labels = np.where(y[order] == 0, 1.0, -1.0)
    A, B = sigmoid_train(dec, labels)
    sv = final['alpha'] > 0
    support = order[sv]
    fit = dict(support=support.astype(np.int32), sv=X[support], dual_coef=(labels * final['alpha'])[sv], intercept=-final['rho'],
               gamma=gamma, probA=A, probB=B, n_support=np.array([(y[support] == 0).sum(), (y[support] == 1).sum()], np.int32),
               n_iter=final['n_iter'], status=final['status'], n_samples=len(y), n_features=X.shape[1])
    return dict(cv=cv, gammas=gammas + [gamma], final=final, order=order, perm=perm, platt=platt, platt_dec=dec, A=A, B=B, fit=fit)
