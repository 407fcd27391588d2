"""CPU restatement (numpy) of the `--train -c LR` fit (mc_lr_fit, k7_lr_fit): what scikit-learn's
LogisticRegression(solver='liblinear', penalty='l1') computes with its defaults (C = 1, tol = 1e-4, fit_intercept,
intercept_scaling = 1, max_iter = 100) through the liblinear scikit-learn vendors -- `solve_l1r_lr` (newGLMNET, Yuan et al. 2011)
behind `train` and `train_one`.  TEST INFRASTRUCTURE: the yardstick the device is held to, never the product.  Line numbers are those
of scikit-learn 1.7's sklearn/svm/src/liblinear/linear.cpp.

* The problem (liblinear_helper.c, linear.cpp:2453-2551): the bias is a constant column of intercept_scaling = 1.0 appended to X
  and penalised like any weight; `group_classes` (:2200-2307, scikit-learn's sorted-label change) puts the classes_[0] rows first,
  stable within each class; in the binary case those rows get y = -1 (:2544-2549), so w points toward classes_[1].  Every row's
  C is C (no class or sample weights).
* Stopping (:2321): eps = tol max(min(pos, neg), 1) / l; at most max_iter Newton iterations, 1000 coordinate-descent sweeps per
  Newton iteration, 20 line-search steps; nu = 1e-12, sigma = 0.01, inner_eps from 1, quartered after a one-sweep inner loop.
  Outer (:1879-1886) and inner (:1949-1956) active-set shrinking as liblinear does them.
* Randomness (:1920-1924): the QP visit order is shuffled with bounded_rand_int (newrand.h: std::mt19937 and Lemire's bounded
  draw) from a generator seeded once per fit with the 31-bit seed -- train_model.MT19937Draws, shared with libsvm's Platt shuffle.
* Sums run over the rows one after another as liblinear's column walk does (dense X with its zeros skipped: the same numbers),
  np.cumsum(v)[-1]; exp and log are the C library's (math.exp, math.log).
"""
import math

import numpy as np

from mcaller_amd.train_model import MT19937Draws

NU, SIGMA = 1e-12, 0.01
MAX_INNER, MAX_LINESEARCH = 1000, 20


def _seq(first, terms):
    """first + terms[0] + terms[1] + ... one after another."""
    return float(np.cumsum(np.concatenate([[first], terms]))[-1]) if len(terms) else float(first)


def _exp(v):
    return np.array([math.exp(a) for a in v])


def liblinear_order(y):
    """The rows as group_classes hands them to the solver: classes_[0] first, then classes_[1], stable within each."""
    y = np.asarray(y)
    return np.concatenate([np.nonzero(y == 0)[0], np.nonzero(y == 1)[0]])


def solve(X, y, seed, C=1.0, tol=1e-4, max_iter=100):
    """solve_l1r_lr on rows X (already in liblinear's order, y in {0, 1}: 0 first) -> dict(w: d+1 weights, the last the bias;
    n_iter: Newton iterations; status: 1 when max_iter was reached)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y)
    l, d = X.shape
    if l == 0 or len(np.unique(y)) != 2 or (np.diff(y.astype(np.int64)) < 0).any():
        raise ValueError('solve: two classes, classes_[0] rows first')
    Xb = np.concatenate([X, np.ones((l, 1))], axis=1)                  # the bias column (liblinear_helper.c)
    n = d + 1
    cols = [np.ascontiguousarray(Xb[:, j]) for j in range(n)]
    neg = y == 0                                                       # y = -1 (:2544-2549)
    pos = int((~neg).sum())
    eps = tol * max(min(pos, l - pos), 1) / l                          # primal_solver_tol (:2321)
    Cr = np.full(l, float(C))
    draws = MT19937Draws(seed)

    w = np.zeros(n)
    wpd = np.zeros(n)
    index = list(range(n))
    w_norm = 0.0
    xjneg_sum = np.array([_seq(0.0, (Cr * cols[j])[neg]) for j in range(n)])      # :1821-1838
    exp_wTx = np.ones(l)                                               # exp(0)  (:1839-1845)
    tau_tmp = 1.0 / (1.0 + exp_wTx)
    tau = Cr * tau_tmp
    D = Cr * exp_wTx * tau_tmp * tau_tmp
    Grad, Hdiag = np.zeros(n), np.zeros(n)
    newton_iter, QP_no_change = 0, 0
    inner_eps, Gnorm1_init, Gmax_old = 1.0, -1.0, math.inf
    xTd = np.zeros(l)

    while newton_iter < max_iter:                                      # :1847
        Gmax_new, Gnorm1_new = 0.0, 0.0
        active_size = n
        s = 0
        while s < active_size:                                         # :1853-1895
            j = index[s]
            Hdiag[j] = _seq(NU, cols[j] * cols[j] * D)
            tmp = _seq(0.0, cols[j] * tau)
            Grad[j] = -tmp + xjneg_sum[j]
            Gp, Gn = Grad[j] + 1, Grad[j] - 1
            violation = 0.0
            if w[j] == 0:
                if Gp < 0:
                    violation = -Gp
                elif Gn > 0:
                    violation = Gn
                elif Gp > Gmax_old / l and Gn < -Gmax_old / l:         # outer-level shrinking
                    active_size -= 1
                    index[s], index[active_size] = index[active_size], index[s]
                    continue
            elif w[j] > 0:
                violation = abs(Gp)
            else:
                violation = abs(Gn)
            Gmax_new = max(Gmax_new, violation)
            Gnorm1_new += violation
            s += 1
        if newton_iter == 0:
            Gnorm1_init = Gnorm1_new
        if Gnorm1_new <= eps * Gnorm1_init or QP_no_change >= 10:     # :1902
            break
        QP_no_change += 1

        it = 0
        QP_Gmax_old = math.inf
        QP_active_size = active_size
        xTd[:] = 0.0
        while it < MAX_INNER:                                          # :1915-2007
            QP_Gmax_new, QP_Gnorm1_new = 0.0, 0.0
            for jj in range(QP_active_size):                           # the shuffle (:1920-1924)
                i = jj + draws.draw(QP_active_size - jj)
                index[i], index[jj] = index[jj], index[i]
            s = 0
            while s < QP_active_size:
                j = index[s]
                H = Hdiag[j]
                G = _seq(Grad[j] + (wpd[j] - w[j]) * NU, cols[j] * D * xTd)
                Gp, Gn = G + 1, G - 1
                violation = 0.0
                if wpd[j] == 0:
                    if Gp < 0:
                        violation = -Gp
                    elif Gn > 0:
                        violation = Gn
                    elif Gp > QP_Gmax_old / l and Gn < -QP_Gmax_old / l:   # inner-level shrinking
                        QP_active_size -= 1
                        index[s], index[QP_active_size] = index[QP_active_size], index[s]
                        continue
                elif wpd[j] > 0:
                    violation = abs(Gp)
                else:
                    violation = abs(Gn)
                if Gp < H * wpd[j]:                                    # the one-variable solution (:1964-1973)
                    z = -Gp / H
                elif Gn > H * wpd[j]:
                    z = -Gn / H
                else:
                    z = -wpd[j]
                if abs(z) < 1.0e-12:
                    s += 1
                    continue
                z = min(max(z, -10.0), 10.0)
                QP_no_change = 0
                QP_Gmax_new = max(QP_Gmax_new, violation)
                QP_Gnorm1_new += violation
                wpd[j] += z
                xTd += cols[j] * z
                s += 1
            it += 1
            if QP_Gnorm1_new <= inner_eps * Gnorm1_init:
                if QP_active_size == active_size:
                    break
                QP_active_size = active_size                           # active set reactivation
                QP_Gmax_old = math.inf
                continue
            QP_Gmax_old = QP_Gmax_new

        delta, w_norm_new = 0.0, 0.0                                   # :2012-2025
        for j in range(n):
            delta += Grad[j] * (wpd[j] - w[j])
            if wpd[j] != 0:
                w_norm_new += abs(wpd[j])
        delta += w_norm_new - w_norm
        negsum_xTd = _seq(0.0, (Cr * xTd)[neg])

        num_linesearch = 0
        while num_linesearch < MAX_LINESEARCH:                         # :2028-2067
            cond = w_norm_new - w_norm + negsum_xTd - SIGMA * delta
            exp_xTd = _exp(xTd)
            exp_wTx_new = exp_wTx * exp_xTd
            r = (1 + exp_wTx_new) / (exp_xTd + exp_wTx_new)
            cond = _seq(cond, Cr * np.array([math.log(a) for a in r]))
            if cond <= 0:
                w_norm = w_norm_new
                w[:] = wpd
                exp_wTx = exp_wTx_new
                tau_tmp = 1 / (1 + exp_wTx)
                tau = Cr * tau_tmp
                D = Cr * exp_wTx * tau_tmp * tau_tmp
                break
            w_norm_new = 0.0
            for j in range(n):
                wpd[j] = (w[j] + wpd[j]) * 0.5
                if wpd[j] != 0:
                    w_norm_new += abs(wpd[j])
            delta *= 0.5
            negsum_xTd *= 0.5
            xTd *= 0.5
            num_linesearch += 1
        if num_linesearch >= MAX_LINESEARCH:                           # :2070-2088 (tau and D stay)
            acc = np.zeros(l)
            for i in range(n):
                if w[i] != 0:
                    acc += w[i] * cols[i]
            exp_wTx = _exp(acc)
        if it == 1:
            inner_eps *= 0.25
        newton_iter += 1
        Gmax_old = Gmax_new
    return dict(w=w.copy(), n_iter=newton_iter, status=1 if newton_iter >= max_iter else 0)


def objective(X, y, w, C=1.0):
    """sum |w_j| + C sum_i log(1 + exp(-y_i w . [x_i, 1])), y_i = -1 for class 0 (any row order)."""
    X = np.asarray(X, dtype=np.float64)
    m = X @ np.asarray(w[:-1]) + w[-1]
    ys = np.where(np.asarray(y) == 0, -1.0, 1.0)
    return float(np.abs(w).sum() + C * np.logaddexp(0.0, -ys * m).sum())


def gradient(X, y, w, C=1.0):
    """The loss part's gradient dL/dw_j (bias last)."""
    X = np.asarray(X, dtype=np.float64)
    Xb = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    ys = np.where(np.asarray(y) == 0, -1.0, 1.0)
    m = Xb @ np.asarray(w)
    return Xb.T @ (-C * ys / (1.0 + np.exp(ys * m)))


def stopping_holds(X, y, w, C=1.0, tol=1e-4):
    """liblinear's stopping test at w: the summed minimum-norm subgradient is at most eps times its value at w = 0."""
    y = np.asarray(y)
    l = len(y)
    pos = int((y == 1).sum())
    eps = tol * max(min(pos, l - pos), 1) / l

    def gnorm1(w):
        G = gradient(X, y, w, C)
        v = np.where(w > 0, np.abs(G + 1), np.where(w < 0, np.abs(G - 1), np.maximum(0.0, np.maximum(-(G + 1), G - 1))))
        return float(v.sum())
    return gnorm1(np.asarray(w, dtype=np.float64)) <= eps * gnorm1(np.zeros(len(w))) * (1 + 1e-6)


def decision(X, w):
    """k3_simple's logistic decision value: the dot product in index order, then the intercept."""
    X = np.asarray(X, dtype=np.float64)
    dec = np.zeros(len(X))
    for f in range(X.shape[1]):
        dec = dec + X[:, f] * w[f]
    return dec + w[-1]


def solve_job(X, y, train, val, seed, **kw):
    """A device job: fit on rows `train` (any order: they are put in liblinear's), score rows `val` (class 1 iff dec > 0)."""
    train = np.asarray(train)
    tr = train[liblinear_order(y[train])]
    out = solve(X[tr], y[tr], seed, **kw)
    dec = decision(X[val], out['w']) if len(val) else np.zeros(0)
    out.update(val_dec=dec, val_correct=int(((dec > 0).astype(np.int64) == y[val]).sum()) if len(val) else 0)
    return out
