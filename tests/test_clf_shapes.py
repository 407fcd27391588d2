"""The references the GPU tests of the RF / LR / NBC / SVM paths trust (tests/test_gpu_clf_shapes.py), pinned at every shape:
a forest walker written from scikit-learn's documented rule against the C oracle on synthetic forests and edge probes
(tests/clf_cases.py), and -- with scikit-learn installed -- the oracles against predict_proba of fitted estimators at 2, 5 and 9
inputs, read back through the model-file loader."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from oracle import clf_oracle
from tests import clf_cases as CC
from tests import helpers as H
from tests import svm_oracle

SHAPES = os.path.join(H.GOLDEN, 'shapes')


def walk_forest(forests, X, sub, cast=True, le=True):
    """predict_proba[:, 1] of a RandomForestClassifier as scikit-learn documents it: X as float32, at each split go left when
    x[feature] <= threshold, the leaf's class weights normalised (a zero sum divides by 1), the mean over the trees in order.
    cast / le: False gives the two mistakes the probes are built to catch (no float32 cast; '<' for '<=')."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X.astype(np.float32).astype(np.float64) if cast else X
    sub = np.asarray(sub)
    p = np.full(len(X), np.nan)
    for m, f in enumerate(forests):
        rows = np.nonzero(sub == m)[0]
        if len(rows) == 0:
            continue
        x = Xc[rows]
        s = np.zeros(len(rows))
        for t in range(f.n_trees):
            node = np.full(len(rows), f.tree_off[t], dtype=np.int64)
            while True:
                inner = f.left[node] >= 0
                if not inner.any():
                    break
                v = x[np.arange(len(rows)), np.where(inner, f.feature[node], 0)]
                thr = f.threshold[node]
                go_left = v <= thr if le else v < thr
                nxt = np.where(go_left, f.left[node], f.right[node])     # (ForestWeights: node numbers over all trees)
                node = np.where(inner, nxt, node)
            v0, v1 = f.value[node, 0], f.value[node, 1]
            norm = (-0.0 + v0) + v1
            norm = np.where(norm == 0.0, 1.0, norm)
            s = s + v1 / norm
        p[rows] = s / f.n_trees
    return p


# ---- forests: the walker, the C oracle, the probes ----

@pytest.mark.parametrize('n_in,n_trees,depth', [(1, (1, 3), (0, 4)), (2, (1, 63, 64), (0, 12)), (5, (65, 7, 130), (0, 20)),
                                                (7, (50, 50), (3, 10)), (9, (64, 65, 2), (0, 20))])
def test_forest_walker_equals_the_c_oracle(n_in, n_trees, depth):
    forests, X, sub = CC.forest_case(100 + n_in, n_in, n_trees, depth)
    want = walk_forest(forests, X, sub)
    got = H.oracle_forest_forward(forests, X, sub)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == (sub == len(forests)).sum()
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])
    # the probes tell the rule apart from the mistakes the GPU tests have to catch
    assert not np.array_equal(walk_forest(forests, X, sub, cast=False)[ok], want[ok])
    assert not np.array_equal(walk_forest(forests, X, sub, le=False)[ok], want[ok])


def test_forest_shapes_are_what_they_say():
    rng = np.random.default_rng(3)
    thr, vals = CC.threshold_pool(rng, 4)
    f = CC.forests(rng, 4, (1, 64, 65, 130), depth=(18, 20), thr=thr, zero_leaf=0.2, single_leaf=0.1)
    assert [w.n_trees for w in f] == [1, 64, 65, 130]
    leaves = np.concatenate([w.left < 0 for w in f])
    vals_ = np.concatenate([w.value for w in f])
    assert ((vals_[leaves].sum(axis=1)) == 0.0).any()                         # zero-sum leaves
    sizes = np.concatenate([np.diff(w.tree_off) for w in f])
    assert (sizes == 1).any() and sizes.max() >= 21                           # single leaves, a path of depth 20
    t = np.concatenate([w.threshold[w.left >= 0] for w in f])
    f32 = t.astype(np.float32).astype(np.float64) == t
    assert f32.any() and (~f32).any()
    for v, tf in zip(vals, thr):                                              # probes on every threshold that is a float32
        assert set(x for x in tf if float(np.float32(x)) == x) <= set(v.tolist())


# ---- the oracles against scikit-learn ----

def sk_forest_probes(rng, f, n):
    """Rows built from a fitted forest's own thresholds: each, its float32 rounding and one float32 ulp either side of that."""
    vals = []
    for j in range(f.n_in):
        t = np.unique(f.threshold[(f.left >= 0) & (f.feature == j)])
        if len(t) == 0:
            t = np.zeros(1)
        t32 = t.astype(np.float32)
        cand = np.concatenate([t, t32, np.nextafter(t32, np.float32(-np.inf)), np.nextafter(t32, np.float32(np.inf))])
        vals.append(cand.astype(np.float64))
    return CC.forest_probes(rng, vals, n)


def sk_round_trip(est, tmp_path, name):
    from mcaller_amd.model_io import load_model_file
    path = os.path.join(str(tmp_path), name)
    with open(path, 'wb') as fh:
        pickle.dump({'MG': est}, fh, protocol=4)
    return load_model_file(path).models['MG']


def sk_rows(rng, n, n_in):
    X = rng.normal(0, 2.0, size=(n, n_in))
    y = np.where(X @ rng.normal(0, 1, n_in) + rng.normal(0, 0.8, n) >= 0, 'm6A', 'A')
    return X, y


@pytest.mark.parametrize('n_in', [2, 5, 9])
def test_forest_oracle_equals_scikit_learn(n_in, tmp_path):
    pytest.importorskip('sklearn')
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(40 + n_in)
    X, y = sk_rows(rng, 300, n_in)
    for n_est, depth in ((1, 10), (50, 10), (65, 10), (130, 10), (20, None)):
        rf = RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=depth, max_features=min(4, n_in), min_samples_leaf=2,
                                    min_samples_split=3, n_estimators=n_est, random_state=3).fit(X, y)
        w = sk_round_trip(rf, tmp_path, 'rf.pkl')
        assert w.kind == 'forest' and w.n_trees == n_est and w.n_in == n_in
        P = np.concatenate([sk_forest_probes(rng, w, 2000), X])
        want = rf.predict_proba(P)[:, 1]
        got = H.oracle_forest_forward([w], P, np.zeros(len(P), dtype=np.uint8))
        assert np.array_equal(got, want), (n_est, depth)


@pytest.mark.parametrize('n_in', [2, 5, 9])
def test_logistic_oracle_equals_scikit_learn(n_in, tmp_path):
    pytest.importorskip('sklearn')
    from sklearn.linear_model import LogisticRegression
    rng = np.random.default_rng(50 + n_in)
    X, y = sk_rows(rng, 300, n_in)
    lr = LogisticRegression(solver='liblinear', penalty='l1', random_state=5).fit(X, y)
    w = sk_round_trip(lr, tmp_path, 'lr.pkl')
    P = CC.logistic_probes(rng, w)
    want = lr.predict_proba(P)[:, 1]
    got = clf_oracle.forward([w], P, np.zeros(len(P), dtype=np.uint8))
    assert (want == 0.0).any() and (want == 1.0).any()
    CC.assert_matches(got, want, 1e-12)
    # decision value 0 exactly: p = 1/2
    w2, x2 = CC.logistic_exact_half(n_in)
    lr.coef_, lr.intercept_ = w2.coef[None, :].copy(), np.array([w2.intercept])
    assert lr.predict_proba(x2)[0, 1] == 0.5 == clf_oracle.forward([w2], x2, np.zeros(1, dtype=np.uint8))[0]


def sk_gnb(theta, var, prior):
    from sklearn.naive_bayes import GaussianNB
    nb = GaussianNB()
    nb.theta_, nb.var_, nb.class_prior_ = np.array(theta, dtype=np.float64), np.array(var, dtype=np.float64), np.array(prior, dtype=np.float64)
    nb.classes_ = np.array(['A', 'm6A'])
    nb.n_features_in_ = nb.theta_.shape[1]
    nb.epsilon_ = 0.0
    return nb


@pytest.mark.parametrize('n_in', [2, 5, 9])
def test_gnb_oracle_equals_scikit_learn(n_in, tmp_path):
    pytest.importorskip('sklearn')
    from sklearn.naive_bayes import GaussianNB
    rng = np.random.default_rng(60 + n_in)
    X, y = sk_rows(rng, 300, n_in)
    fitted = GaussianNB().fit(X, y)
    tiny = CC.gnb_tiny_var(rng, n_in)
    tie, x_tie = CC.gnb_tie(rng, n_in)
    far, x_far = CC.gnb_tie(rng, n_in, var=1e-6)
    for nb in (fitted, sk_gnb(tiny.theta, tiny.var, tiny.prior), sk_gnb(tie.theta, tie.var, tie.prior), sk_gnb(far.theta, far.var, far.prior)):
        w = sk_round_trip(nb, tmp_path, 'nb.pkl')
        P = np.concatenate([CC.gnb_probes(rng, w), x_tie if nb.theta_ is not fitted.theta_ else X[:20]])
        if nb.theta_[0, 0] == far.theta[0, 0]:
            P = np.concatenate([P, x_far, CC.gnb_near_tie_probes(rng, far, x_far)])
            mid = nb.predict_proba(P[-40:])[:, 1]
            assert ((mid > 0.05) & (mid < 0.95)).sum() >= 10          # p in the middle, |jll| in the millions
        want = nb.predict_proba(P)[:, 1]
        got = clf_oracle.forward([w], P, np.zeros(len(P), dtype=np.uint8))
        CC.assert_matches(got, want, 1e-12)
    # at the tie the two jll are equal bit for bit: p is 1/2 up to the rounding of logsumexp, and the oracle rounds the same way
    p_tie = sk_gnb(tie.theta, tie.var, tie.prior).predict_proba(x_tie)[0, 1]
    assert abs(p_tie - 0.5) <= 1e-15 and clf_oracle.forward([tie], x_tie, np.zeros(1, dtype=np.uint8))[0] == p_tie
    w = CC.gnb_tiny_var(rng, n_in)
    p = sk_gnb(w.theta, w.var, w.prior).predict_proba(CC.gnb_probes(rng, w))[:, 1]
    assert (p == 0.0).any() and (p == 1.0).any()


@pytest.mark.parametrize('n_in', [2, 5, 9])
def test_svm_oracle_equals_scikit_learn(n_in, tmp_path):
    pytest.importorskip('sklearn')
    from sklearn.svm import SVC
    rng = np.random.default_rng(70 + n_in)
    X, y = sk_rows(rng, 200, n_in)
    svc = SVC(kernel='rbf', probability=True, random_state=7).fit(X, y)
    w = sk_round_trip(svc, tmp_path, 'svm.pkl')
    assert w.kind == 'svm' and w.n_in == n_in
    P = np.concatenate([CC.svm_band_probes(rng, w), X[:50], rng.normal(0, 30.0, size=(20, n_in))])
    want = svc.predict_proba(P)[:, 1]
    got = svm_oracle.forward([w], P, np.zeros(len(P), dtype=np.uint8))
    assert (want == 0.5).sum() >= 2
    CC.assert_matches(got, want, 1e-11)


def test_svm_probes_reach_the_band_and_the_clamp():
    rng = np.random.default_rng(8)
    w = CC.svm_scaled(rng, 5, 300)
    P = CC.svm_band_probes(rng, w)
    assert len(P) == len(CC.SVM_F_TARGETS)
    s = svm_oracle.pairwise(svm_oracle.decision(w.sv, w.dual_coef, w.gamma, w.intercept, P), w.A, w.B)
    p = svm_oracle.couple2(s)
    assert (p == 0.5).sum() == 5                                   # 0, +-0.005, +-0.0199
    assert ((s == 1e-7) | (s == 1.0 - 1e-7)).sum() >= 4             # +-16.3, +-25: clamped
    assert ((s > 1e-7) & (s < 2e-7)).any()                          # +-16: not yet


# ---- the committed five-input model files ----

def test_shape_fixtures_load_without_sklearn(monkeypatch):
    from mcaller_amd.model_io import load_model_file
    for name in list(sys.modules):
        if name == 'sklearn' or name.startswith('sklearn.'):
            monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, 'sklearn', None)
    meta = json.load(open(os.path.join(SHAPES, 'shapes_meta.json')))
    kinds = {'RF': 'forest', 'RF4': 'forest', 'LR': 'logistic', 'NBC': 'gnb', 'SVM': 'svm'}
    for tag, kind in kinds.items():
        ms = load_model_file(os.path.join(SHAPES, 'shapes_twobase_model_%s_4_m6A.pkl' % tag))
        assert ms.twobase and ms.keys() == ['MG', 'MH']
        assert all(w.kind == kind and w.n_in == meta['n_in'] == 5 for w in ms.models.values())
        if kind == 'forest':
            assert all(w.n_trees == meta['n_trees'][tag] for w in ms.models.values())


def test_shape_generator_reproduces_the_committed_fixtures(tmp_path):
    sklearn = pytest.importorskip('sklearn')
    meta = json.load(open(os.path.join(SHAPES, 'shapes_meta.json')))
    if sklearn.__version__ != meta['sklearn']:
        pytest.skip('fixtures were made with scikit-learn %s, this is %s' % (meta['sklearn'], sklearn.__version__))
    r = subprocess.run([sys.executable, os.path.join(H.GOLDEN, 'make_golden_shapes.py'), '--out', str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=H.REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    made = tmp_path / 'tests' / 'golden' / 'shapes'
    names = sorted(os.listdir(made))
    assert names == sorted(os.listdir(SHAPES))
    for name in names:
        assert (made / name).read_bytes() == open(os.path.join(SHAPES, name), 'rb').read(), name
