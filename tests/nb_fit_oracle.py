"""CPU restatement (numpy) of the `--train -c NBC` fit (mc_nb_fit, k7_nb_fit): what scikit-learn's GaussianNB() computes in its first
partial fit.  TEST INFRASTRUCTURE: the yardstick the device is held to, never the product.

* Per class (classes_ = [0, 1]): the row count, the mean and the centred (two-pass) variance of every feature, each sum over the
  rows one after another (numpy's reduction along axis 0).
* epsilon_ = var_smoothing * max_f var(X_train[:, f]), added to every variance; class_prior_ = count / n.
* Prediction: argmax of the joint log-likelihood log prior - 0.5 sum log(2 pi var) - 0.5 sum (x - theta)^2 / var, ties to class 0.
"""
import numpy as np


def _var(X):
    mean = np.sum(X, axis=0) / len(X)
    return mean, np.sum((X - mean) ** 2, axis=0) / len(X)


def fit(X, y, var_smoothing=1e-9):
    """-> dict(theta [2, d], var [2, d], epsilon, class_count [2], class_prior [2])."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y)
    eps = var_smoothing * _var(X)[1].max()
    theta, var = np.zeros((2, X.shape[1])), np.zeros((2, X.shape[1]))
    for c in (0, 1):
        theta[c], var[c] = _var(X[y == c])
    count = np.array([(y == 0).sum(), (y == 1).sum()], dtype=np.float64)
    return dict(theta=theta, var=var + eps, epsilon=float(eps), class_count=count, class_prior=count / count.sum())


def joint_log_likelihood(m, X):
    X = np.asarray(X, dtype=np.float64)
    out = []
    for c in (0, 1):
        n_ij = -0.5 * np.sum(np.log(2.0 * np.pi * m['var'][c]))
        out.append(np.log(m['class_prior'][c]) + n_ij - 0.5 * np.sum(((X - m['theta'][c]) ** 2) / m['var'][c], axis=1))
    return np.stack(out, axis=1)


def predict(m, X):
    jll = joint_log_likelihood(m, X)
    return (jll[:, 1] > jll[:, 0]).astype(np.int64)


def fit_job(X, y, train, val, var_smoothing=1e-9):
    """A device job: fit on rows `train`, count the right predictions on rows `val` (and the joint log-likelihood gap there)."""
    out = fit(X[train], y[train], var_smoothing)
    if len(val):
        jll = joint_log_likelihood(out, X[val])
        out.update(val_gap=jll[:, 1] - jll[:, 0], val_correct=int((predict(out, X[val]) == y[val]).sum()))
    else:
        out.update(val_gap=np.zeros(0), val_correct=0)
    return out
