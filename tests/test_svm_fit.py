"""The `--train -c SVM` fit's CPU restatement (tests/svm_fit_oracle.py) against scikit-learn's SVC, and the writers and loader of
the fitted model.  No GPU: the device is held to the oracle in tests/test_gpu_svm_fit.py."""
import pickle

import numpy as np
import pytest

from tests import svm_fit_oracle as so
from tests import svm_oracle
from tests.helpers import block_sklearn

BAND = 5e-3


def data(n, d, seed, kind='plain'):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * np.linspace(0.5, 3.0, d)
    if kind == 'rounded':                                   # heavy duplicates
        X = np.round(X, 0)
    if kind == 'const' and d > 1:
        X[:, -1] = 7.25
    z = X[:, 0] - 0.7 * X[:, min(1, d - 1)] + 0.3 * np.sin(3 * X[:, min(2, d - 1)])
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-2.0 * z))).astype(np.uint8)
    return X, y


def sk_labels(y):
    return np.array(['A', 'm6A'])[y]


def compare_to_sklearn(X, y, probe, unique_rows=True):
    """The oracle's solve on all rows (classes_[0] first) against SVC(C=1, gamma) fitted by scikit-learn on the same rows.  With
    repeated rows the dual's optimum is not unique (alpha may be shared among copies): the support sets are compared only without."""
    from sklearn.svm import SVC
    order = so.grouped(np.arange(len(y)), y, 0)
    g = so.gamma_of(X)
    ys = np.where(y[order] == 0, 1.0, -1.0)
    s = so.smo(X[order], ys, g)
    sk = SVC(C=1.0, gamma=g).fit(X[order], sk_labels(y[order]))
    assert so.kkt_violation(X[order], ys, s['alpha'], g) <= 1e-3
    sv = s['alpha'] > 0
    ours = so.dual_objective(X[order][sv], (ys * s['alpha'])[sv], g)
    theirs = so.dual_objective(sk.support_vectors_, sk._dual_coef_, g)
    assert abs(ours - theirs) <= 1e-6 * abs(theirs)
    dec = svm_oracle.decision(X[order][sv], (ys * s['alpha'])[sv], g, -s['rho'], probe)
    want = -sk.decision_function(probe)                      # (libsvm's sign: > 0 is classes_[0])
    assert np.abs(dec - want).max() <= BAND
    sure = np.abs(want) >= BAND
    assert ((dec > 0) == (want > 0))[sure].all()
    a, b = set(order[sv].tolist()), set(order[sk.support_].tolist())
    assert not unique_rows or len(a ^ b) <= max(1, 0.01 * len(b)), (len(a ^ b), len(b))
    return s


@pytest.mark.parametrize('n,d,kind', [(40, 1, 'plain'), (40, 4, 'rounded'), (300, 4, 'plain'), (300, 7, 'const'),
                                      (2000, 7, 'plain'), (2000, 9, 'rounded'), (5000, 7, 'plain'), (5000, 1, 'plain')])
def test_the_oracle_solve_equals_sklearn(n, d, kind):
    pytest.importorskip('sklearn')
    X, y = data(n, d, n + d, kind)
    if kind == 'rounded':
        X[: n // 4] = X[n // 4: 2 * (n // 4)]                # (duplicated rows, some with the other label)
    probe, _ = data(2000, d, 99, kind)
    s = compare_to_sklearn(X, y, probe, len(np.unique(X, axis=0)) == n)
    assert s['status'] == 0 and s['n_iter'] > 0


def test_a_constant_matrix_has_gamma_one_and_the_iteration_cap_reports_a_status():
    X = np.full((30, 3), 2.5)
    y = np.arange(30) % 2
    assert so.gamma_of(X) == 1.0
    ys = np.where(y == 0, 1.0, -1.0)
    s = so.smo(X, ys, 1.0)
    assert s['status'] == 0
    X2, y2 = data(300, 4, 3)
    s = so.smo(X2, np.where(y2 == 0, 1.0, -1.0), so.gamma_of(X2), max_iter=5)
    assert s['status'] == 1 and s['n_iter'] == 5


def cv_setup(n, d, seed):
    from mcaller_amd import train_model
    X, y = data(n, d, seed)
    labs = list(sk_labels(y))
    grps = ['g%d' % (i % 37) for i in range(n)]
    classes, yy, jobs, seeds = train_model.cv_jobs(labs, grps, True)
    assert (yy == y).all()
    return X, y, labs, grps, jobs, seeds


def test_fold_gammas_equal_sklearn_clones_bit_for_bit():
    pytest.importorskip('sklearn')
    from sklearn.svm import SVC
    from mcaller_amd import train_model
    for n, d in ((300, 7), (2000, 4), (911, 9)):
        X, y, labs, grps, jobs, seeds = cv_setup(n, d, n)
        for tr, va in jobs:
            sk = SVC(C=1.0).fit(X[tr], sk_labels(y[tr]))
            assert so.gamma_of(X[tr]) == sk._gamma and train_model.svc_gamma(X[tr]) == sk._gamma
        plan = train_model.svm_plan(X, y, jobs, seeds[5])
        assert plan['gammas'][:5] == [so.gamma_of(X[tr]) for tr, _ in jobs[:5]] and plan['gamma'] == so.gamma_of(X)


def test_cv_scores_equal_cross_val_score_outside_the_band():
    pytest.importorskip('sklearn')
    from sklearn.model_selection import GroupKFold, cross_val_score
    from sklearn.svm import SVC
    X, y, labs, grps, jobs, seeds = cv_setup(1500, 7, 8)
    want = cross_val_score(SVC(kernel='rbf'), X, labs, cv=GroupKFold(n_splits=5), groups=grps)   # (predict ignores Platt)
    near = 0
    for f, (tr, va) in enumerate(jobs[:5]):
        s = so.solve_job(X, y, so.grouped(tr, y, 0), va, so.gamma_of(X[tr]))
        sk = SVC(C=1.0).fit(X[tr], sk_labels(y[tr]))
        assert sk.score(X[va], sk_labels(y[va])) == want[f]
        pred = np.where(s['val_dec'] > 0, 0, 1)
        skp = (sk.predict(X[va]) == 'm6A').astype(int)
        band = np.abs(s['val_dec']) < BAND
        assert (pred == skp)[~band].all()
        near += int(band.sum())
        assert abs(s['val_correct'] / len(va) - want[f]) <= band.sum() / len(va)
    assert near <= 10


def one_class_fold_seed(y, order):
    """A seed whose shuffle puts every classes_[1] row of `order` into one fold (its complement then holds one class)."""
    l = len(order)
    for R in range(2000):
        seed = np.random.RandomState(R).randint(2 ** 31 - 1)
        perm = so.permutation(l, seed)
        for f in range(5):
            comp = order[np.concatenate([perm[:f * l // 5], perm[(f + 1) * l // 5:]])]
            if (y[comp] == 0).all():
                return R
    raise AssertionError('no seed found')


@pytest.mark.parametrize('n,R', [(300, 3), (1000, 7), (1000, 11), (2000, 1), (12, None)])
def test_platt_pin_reproduces_sklearn_probA_probB_bit_for_bit(n, R):
    """Given the seed scikit-learn hands libsvm (RandomState(R).randint(2**31 - 1)): the oracle's shuffle, SVC sub-fits on the
    fold complements in libsvm's order, and sigmoid_train give probA_ and probB_ exactly.  n = 12 (ten rows of one class): a fold
    whose complement holds one class, dec = +1 on its rows."""
    pytest.importorskip('sklearn')
    from sklearn.svm import SVC
    X, y = data(n, 4, n)
    if R is None:
        y = np.zeros(n, dtype=np.uint8)
        y[[3, 8]] = 1
        R = one_class_fold_seed(y, so.grouped(np.arange(n), y, 0))
    est = SVC(kernel='rbf', probability=True, random_state=R).fit(X, sk_labels(y))
    seed = np.random.RandomState(R).randint(2 ** 31 - 1)
    order = so.grouped(np.arange(n), y, 0)
    perm = so.permutation(n, seed)
    dec = np.zeros(n)
    consts = 0
    for f in range(5):
        b, e = f * n // 5, (f + 1) * n // 5
        comp = order[np.concatenate([perm[:b], perm[e:]])]
        held = perm[b:e]
        if len(set(y[comp].tolist())) < 2:
            dec[held] = 1.0 if y[comp][0] == 0 else -1.0
            consts += 1
            continue
        sub = SVC(C=1.0, gamma=est._gamma).fit(X[comp], np.where(y[comp] == 0, 1, -1))
        dec[held] = sub.decision_function(X[order[held]])
    A, B = so.sigmoid_train(dec, np.where(y[order] == 0, 1.0, -1.0))
    assert A == est.probA_[0] and B == est.probB_[0]
    assert consts == (1 if n == 12 else 0)


def test_permutation_of_the_product_equals_the_oracle():
    from mcaller_amd import train_model
    for l in (1, 2, 5, 37, 1000, 9244):
        for seed in (0, 1, 77, 2 ** 31 - 2):
            assert (train_model.libsvm_permutation(l, seed) == so.permutation(l, seed)).all()
    assert train_model.platt_seed(2 ** 64 - 1) == so.platt_seed(2 ** 64 - 1) < 2 ** 31 - 1


def _oracle_fit(n=400, d=7, seed=5):
    from mcaller_amd import train_model
    X, y, labs, grps, jobs, seeds = cv_setup(n, d, seed)
    sub = so.fit_submodel(X, y, jobs, seeds[5])
    plan = train_model.svm_plan(X, y, jobs, seeds[5])
    assert (plan['perm'] == sub['perm']).all() and (plan['order'] == sub['order']).all()
    return X, y, labs, sub


def test_as_sklearn_svc_round_trips_and_carries_every_attribute():
    pytest.importorskip('sklearn')
    from sklearn.svm import SVC
    from mcaller_amd.model_io import SVMWeights
    from mcaller_amd.train_model import as_sklearn_svc
    X, y, labs, sub = _oracle_fit()
    est = pickle.loads(pickle.dumps(as_sklearn_svc(sub['fit'], ['A', 'm6A'])))
    fit = sub['fit']
    w = SVMWeights(fit['sv'], fit['dual_coef'], fit['gamma'], fit['intercept'], fit['probA'], fit['probB'])
    probe, _ = data(3000, 7, 21)
    assert np.abs(est.predict_proba(probe)[:, 1] - svm_oracle.proba(w, probe)).max() <= 1e-12
    assert (est.support_vectors_ == X[est.support_]).all()
    ref = SVC(kernel='rbf', probability=True).fit(X, labs)
    mine, theirs = vars(est), vars(ref)
    assert sorted(mine) == sorted(theirs)
    for k, v in theirs.items():
        assert type(mine[k]) is type(v), k
        if isinstance(v, np.ndarray):
            assert mine[k].dtype == v.dtype and mine[k].ndim == v.ndim, k
            if k not in ('support_', 'support_vectors_', '_dual_coef_', 'dual_coef_'):
                assert mine[k].shape == v.shape, k
    assert est.dual_coef_.shape[1] == len(est.support_) == est._n_support.sum()
    assert (est.dual_coef_ == -est._dual_coef_).all() and (est.intercept_ == -est._intercept_).all()
    assert est.predict(probe[:5]).dtype == ref.predict(probe[:5]).dtype


def test_the_svm_npz_round_trips_through_model_io(tmp_path, monkeypatch):
    from mcaller_amd.model_io import load_model_file
    from mcaller_amd.train_model import write_models
    X, y, labs, sub = _oracle_fit(300, 4, 9)
    block_sklearn(monkeypatch)
    path = str(tmp_path / 'm.npz')
    write_models({'general': sub['fit'], 'AC': sub['fit']}, {'general': ['A', 'm6A'], 'AC': ['A', 'm6A']}, {}, path, 'SVM')
    assert open(path, 'rb').read(2) == b'PK'
    ms = load_model_file(path)
    assert ms.twobase and sorted(ms.keys()) == ['AC', 'general']
    w = ms.models['general']
    fit = sub['fit']
    assert w.kind == 'svm' and w.classes == ['A', 'm6A'] and w.n_in == 4
    assert (w.sv == fit['sv']).all() and (w.dual_coef == fit['dual_coef']).all()
    assert (w.gamma, w.intercept, w.A, w.B) == (fit['gamma'], fit['intercept'], fit['probA'], fit['probB'])
