"""CPU restatement (numpy) of scikit-learn's `SVC(kernel='rbf', probability=True).predict_proba` for two classes -- what the
reference's `-c SVM` model files (train_model.py:51-53) are scored with at extract_contexts.py:199.  TEST INFRASTRUCTURE: the
check that k3_svm is held to, never the product.

scikit-learn hands the fitted model to its copy of libsvm (svm_predict_probability); restated from that published algorithm:

* dec = sum_i _dual_coef_[0][i] * exp(-_gamma * sum_j (x_j - sv_ij)^2) + _intercept_[0], the support vectors in order (libsvm's
  k_function and svm_predict_values; `_intercept_` is -rho).
* s = sigmoid_predict(dec, probA, probB) clamped to [1e-7, 1 - 1e-7] -- the pairwise probability of classes_[0] over classes_[1].
* multiclass_probability(k=2, r) -- libsvm runs the iterative coupling even for two classes; the score is p[1] (classes_[1]).

Pinned by tests/golden/svm/svm_meta.json (scikit-learn's own predict_proba, tests/golden/make_golden_svm.py)."""
import numpy as np


def decision(sv, dual_coef, gamma, intercept, X):
    """libsvm's decision value of every row of X, the products added in support-vector order."""
    X = np.asarray(X, dtype=np.float64)
    sv = np.asarray(sv, dtype=np.float64)
    coef = np.asarray(dual_coef, dtype=np.float64).reshape(-1)
    dec = np.zeros(len(X))
    for i in range(len(sv)):
        d = X - sv[i]
        s = np.zeros(len(X))
        for j in range(sv.shape[1]):            # (x_j - sv_ij)^2 added feature by feature, as k_function does
            s = s + d[:, j] * d[:, j]
        dec = dec + coef[i] * np.exp(-gamma * s)
    return dec + intercept


def pairwise(dec, A, B):
    """sigmoid_predict and the clamp of svm_predict_probability: P(classes_[0]) from the decision value."""
    f = np.asarray(dec, dtype=np.float64) * A + B
    s = np.empty_like(f)
    pos = f >= 0
    e = np.exp(-f[pos])
    s[pos] = e / (1.0 + e)
    s[~pos] = 1.0 / (1.0 + np.exp(f[~pos]))
    return np.minimum(np.maximum(s, 1e-7), 1.0 - 1e-7)


def couple2(s):
    """multiclass_probability for k = 2, r01 = s, r10 = 1 - s -> p[1].  libsvm's loop for every row at once: a row stops updating
    at the iteration whose error test it passes (the same operations, element by element, as the row alone would do)."""
    r01 = np.asarray(s, dtype=np.float64)
    r10 = 1.0 - r01
    Q = [[r10 * r10, -r10 * r01], [-r10 * r01, r01 * r01]]
    p = [np.full(len(r01), 0.5), np.full(len(r01), 0.5)]
    eps = 0.005 / 2
    live = np.ones(len(r01), dtype=bool)
    for _ in range(100):
        Qp = [Q[0][0] * p[0] + Q[0][1] * p[1], Q[1][0] * p[0] + Q[1][1] * p[1]]
        pQp = p[0] * Qp[0] + p[1] * Qp[1]
        live &= ~(np.maximum(np.abs(Qp[0] - pQp), np.abs(Qp[1] - pQp)) < eps)
        if not live.any():
            break
        for t in range(2):
            diff = np.where(live, (-Qp[t] + pQp) / Q[t][t], 0.0)
            p[t] = np.where(live, p[t] + diff, p[t])
            pQp = (pQp + diff * (diff * Q[t][t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(2):
                Qp[j] = (Qp[j] + diff * Q[t][j]) / (1 + diff)
                p[j] = np.where(live, p[j] / (1 + diff), p[j])
    return p[1]


def proba(w, X):
    """predict_proba(X)[:, 1] of one model_io.SVMWeights."""
    return couple2(pairwise(decision(w.sv, w.dual_coef, w.gamma, w.intercept, X), w.A, w.B))


def forward(models, X, submodel):
    """models: list of SVMWeights; submodel[i]: which of them scores row i (>= len: NaN)."""
    X = np.asarray(X, dtype=np.float64)
    sub = np.asarray(submodel)
    p = np.full(len(X), np.nan)
    for i, m in enumerate(models):
        sel = sub == i
        if sel.any():
            p[sel] = proba(m, X[sel])
    return p
