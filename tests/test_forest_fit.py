"""The random-forest fit's CPU restatement (tests/forest_fit_oracle.py) against scikit-learn -- exactly where scikit-learn's own
randomness cannot matter, statistically where it can -- and the model files `--train -c RF` writes (no GPU needed)."""
import pickle

import numpy as np
import pytest

from tests import forest_fit_oracle as fo
from tests.helpers import block_sklearn

LEAF_MIN = fo.REFERENCE['min_samples_leaf']


def one_feature(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 3000))
    kind = seed % 5
    x = rng.normal(size=n)
    if kind == 1:
        x = np.round(x, 1)                                                  # many repeats
    elif kind == 2:
        x = 1.0 + rng.integers(0, 6, n) * 1.2e-7 * rng.choice([0.5, 1.0, 2.0], n)   # a few float32 ulps apart near 1.0
    elif kind == 3:
        x = x * 1e3
    elif kind == 4:
        n = int(rng.integers(20, 60))                                       # small: splits rejected by min_samples_leaf, pure nodes
        x = np.round(rng.normal(size=n), 0)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-2.0 * (x - x.mean()) / (np.std(x) + 1e-12)))).astype(np.int64)
    return x[:n].reshape(-1, 1), y


@pytest.mark.parametrize('seed', range(20))
def test_one_feature_trees_equal_sklearn_node_for_node(seed):
    """d = 1: the feature draw is trivial, so a tree on the bootstrap counts (as sample_weight) is scikit-learn's own."""
    DecisionTreeClassifier = pytest.importorskip('sklearn.tree').DecisionTreeClassifier
    X, y = one_feature(seed)
    n = len(y)
    tk = fo.tree_key(seed, 0)
    w = fo.bootstrap_weights(np.arange(n), n, tk)
    tree = fo.fit_tree(X.astype(np.float32), y, w, fo.g_table(n), tk, max_features=1)
    m = w > 0
    clf = DecisionTreeClassifier(criterion='entropy', max_depth=10, min_samples_leaf=2, min_samples_split=3)
    clf.fit(X[m], y[m], sample_weight=w[m].astype(np.float64))
    T = clf.tree_
    assert T.node_count == len(tree['left'])
    assert (T.children_left == tree['left']).all() and (T.children_right == tree['right']).all()
    assert (T.feature == tree['feature']).all()
    assert (T.threshold.view(np.uint64) == tree['threshold'].view(np.uint64)).all()
    assert (T.n_node_samples == tree['n_node_samples']).all()
    assert (T.weighted_n_node_samples == tree['weighted_n_node_samples']).all()
    assert np.abs(T.value[:, 0, :] - tree['value']).max() <= 1e-15
    assert np.abs(T.impurity - tree['impurity']).max() <= 1e-12


def test_one_feature_cases_reach_the_edges():
    """The seeded sets above hold what they are there for: the depth limit, pure leaves, leaves too small to split."""
    depth_hit = pure = small = 0
    for seed in range(20):
        X, y = one_feature(seed)
        n = len(y)
        tk = fo.tree_key(seed, 0)
        w = fo.bootstrap_weights(np.arange(n), n, tk)
        tr = fo.fit_tree(X.astype(np.float32), y, w, fo.g_table(n), tk, max_features=1)
        depth = node_depths(tr)
        leaf = tr['left'] < 0
        depth_hit += int((depth[leaf] == 10).any())
        pure += int((leaf & ((tr['value'][:, 0] == 0) | (tr['value'][:, 1] == 0))).any())
        small += int((leaf & (tr['n_node_samples'] < 3)).any())
    assert depth_hit and pure and small


def node_depths(tr):
    depth = np.zeros(len(tr['left']), dtype=np.int64)
    for v in range(len(tr['left'])):
        if tr['left'][v] >= 0:
            depth[tr['left'][v]] = depth[tr['right'][v]] = depth[v] + 1
    return depth


def seven_features(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 7)) * np.array([1.0, 2.0, 0.5, 3.0, 1.0, 0.2, 1.0])
    X[:, 6] = 7.0 + 0.25 * rng.integers(0, 8, n)                           # read quality: few values, constant in small nodes
    X[:, 3] = np.round(X[:, 3], 1)
    z = 0.9 * X[:, 0] - 0.5 * X[:, 1] + np.sin(2.0 * X[:, 2]) + 0.3 * X[:, 3] * X[:, 4]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.int64)
    return X, y


def test_seven_feature_forests_hold_the_rules():
    """Every split valid (rules 4-6), the best over the node's visited features by brute force, children's weights summing to
    their parent's, values summing to 1, depth <= 10."""
    X, y = seven_features(1500, 3)
    X32 = X.astype(np.float32)
    G = fo.g_table(len(y))
    n_split = 0
    for t in range(4):
        tk = fo.tree_key(11, t)
        w = fo.bootstrap_weights(np.arange(len(y)), len(y), tk)
        trace = []
        tr = fo.fit_tree(X32, y, w, G, tk, trace=trace)
        assert np.abs(tr['value'].sum(axis=1) - 1.0).max() <= 1e-15
        assert node_depths(tr).max() <= 10
        members = {0: np.nonzero(w > 0)[0]}
        for v in range(len(tr['left'])):                                 # pre-order: a node's rows are known before it is visited
            idx = members[v]
            assert tr['n_node_samples'][v] == len(idx) and tr['weighted_n_node_samples'][v] == w[idx].sum()
            if tr['left'][v] < 0:
                continue
            f, t_ = tr['feature'][v], tr['threshold'][v]
            go = X32[idx, f].astype(np.float64) <= t_
            members[tr['left'][v]], members[tr['right'][v]] = idx[go], idx[~go]
            assert go.sum() >= LEAF_MIN and (~go).sum() >= LEAF_MIN and len(idx) >= 3
            assert tr['weighted_n_node_samples'][tr['left'][v]] + tr['weighted_n_node_samples'][tr['right'][v]] == \
                tr['weighted_n_node_samples'][v]
        for v, visited in trace:
            idx = members[v]
            got = split_score(X32, y, w, idx, tr['feature'][v], tr['threshold'][v], G)
            for f in visited:
                xs = np.unique(X32[idx, f].astype(np.float64))
                for a, b in zip(xs[:-1], xs[1:]):
                    if b <= a + fo.THR:
                        continue
                    go = X32[idx, f].astype(np.float64) <= a
                    if go.sum() < LEAF_MIN or (~go).sum() < LEAF_MIN:
                        continue
                    assert split_score(X32, y, w, idx, f, a, G) <= got
            n_split += 1
    assert n_split > 50


def split_score(X32, y, w, idx, f, t, G):
    go = X32[idx, f].astype(np.float64) <= t
    c = [[int(w[idx][go & (y[idx] == k)].sum()) for k in (0, 1)], [int(w[idx][~go & (y[idx] == k)].sum()) for k in (0, 1)]]
    return ((G[c[0][0]] + G[c[0][1]]) - G[sum(c[0])]) + ((G[c[1][0]] + G[c[1][1]]) - G[sum(c[1])])


def test_forests_behave_like_sklearn_random_forests():
    """Config 5's shape (9 244 balanced rows, 7 features, GroupKFold by context): cross-validation accuracy, held-out
    probabilities and tree sizes against RandomForestClassifier with the reference's settings."""
    sk = pytest.importorskip('sklearn.ensemble')
    from sklearn.model_selection import GroupKFold
    X, y = seven_features(9244, 21)
    groups = np.random.default_rng(5).integers(0, 200, len(y))
    folds = list(GroupKFold(n_splits=5).split(X, y, groups))
    ours, theirs, dp, nodes_o, nodes_s = [], [], [], [], []
    for k, (tr, va) in enumerate(folds):
        trees = fo.fit_forest(X, y, tr, 1000 + k)
        _, p = fo.predict_proba(trees, X[va])
        rf = sk.RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=10, max_features=4, min_samples_leaf=2,
                                       min_samples_split=3, n_estimators=50, random_state=k).fit(X[tr], y[tr])
        q = rf.predict_proba(X[va])[:, 1]
        ours.append(((p > 0.5) == y[va]).mean())
        theirs.append(((q > 0.5) == y[va]).mean())
        dp.append(np.abs(p - q).mean())
        nodes_o.append(np.mean([len(t['left']) for t in trees]))
        nodes_s.append(np.mean([e.tree_.node_count for e in rf.estimators_]))
        if k == 1:
            break                                               # (two folds hold the comparison; the rest add minutes, not evidence)
    assert abs(np.mean(ours) - np.mean(theirs)) <= 0.02
    assert np.mean(dp) <= 0.05
    assert abs(np.mean(nodes_o) / np.mean(nodes_s) - 1.0) <= 0.15


def as_fit(trees, d):
    """The oracle's trees in Device.forest_fit's layout."""
    fit = {k: np.concatenate([t[k] for t in trees]) for k in trees[0]}
    fit['tree_off'] = np.cumsum([0] + [len(t['left']) for t in trees])
    fit['n_features'] = d
    return fit


@pytest.fixture(scope='module')
def small_forest():
    X, y = seven_features(800, 8)
    trees = fo.fit_forest(X, y, np.arange(len(y)), 42, n_trees=12)
    return X, trees


def test_written_pickle_is_a_sklearn_forest_and_loads_without_sklearn(small_forest, tmp_path, monkeypatch):
    pytest.importorskip('sklearn')
    from mcaller_amd import train_model
    from mcaller_amd.model_io import load_model_file
    X, trees = small_forest
    path = str(tmp_path / 'rf.pkl')
    train_model.write_models({'general': as_fit(trees, 7)}, {'general': ['A', 'm6A']}, {'general': len(X)}, path, 'RF')
    with open(path, 'rb') as fh:
        rf = pickle.load(fh)['general']
    _, p1 = fo.predict_proba(trees, X)
    P = rf.predict_proba(X)
    assert (P[:, 1] == p1).all() and list(rf.classes_) == ['A', 'm6A']
    assert all(e.tree_.node_count == len(t['left']) for e, t in zip(rf.estimators_, trees))
    block_sklearn(monkeypatch)
    ms = load_model_file(path)
    w = ms.models['general']
    assert ms.twobase and w.kind == 'forest' and w.n_trees == 12 and w.n_in == 7 and w.classes == ['A', 'm6A']
    assert (w.feature == np.concatenate([t['feature'] for t in trees])).all()


def test_npz_written_without_sklearn_loads_to_the_same_forest(small_forest, tmp_path, monkeypatch):
    from mcaller_amd import train_model
    from mcaller_amd.model_io import load_model_file
    X, trees = small_forest
    want = None
    try:
        import sklearn  # noqa: F401
        pk = str(tmp_path / 'rf.pkl')
        train_model.write_models({'general': as_fit(trees, 7)}, {'general': ['A', 'm6A']}, {'general': len(X)}, pk, 'RF')
        want = load_model_file(pk).models['general']
    except ImportError:
        pass
    block_sklearn(monkeypatch)
    path = str(tmp_path / 'rf_model')
    train_model.write_models({'general': as_fit(trees, 7)}, {'general': ['A', 'm6A']}, {'general': len(X)}, path, 'RF')
    assert open(path, 'rb').read(2) == b'PK'
    ms = load_model_file(path)
    w = ms.models['general']
    assert ms.twobase and w.kind == 'forest' and w.n_trees == 12 and w.n_in == 7 and w.classes == ['A', 'm6A']
    base = np.repeat(w.tree_off[:-1], np.diff(w.tree_off))
    left = np.concatenate([t['left'] for t in trees])
    assert (w.left == np.where(left >= 0, left + base, -1)).all()
    assert (w.threshold == np.concatenate([t['threshold'] for t in trees])).all()
    assert (w.value == np.concatenate([t['value'] for t in trees])).all()
    if want is not None:
        for f in ('tree_off', 'left', 'right', 'feature', 'threshold', 'value'):
            assert (getattr(w, f) == getattr(want, f)).all()
        assert (w.n_in, w.n_trees, w.classes) == (want.n_in, want.n_trees, want.classes)
    # an MLP export still loads as before
    from mcaller_amd.model_io import shipped_model
    assert load_model_file(shipped_model('r95_twobase_model_NN_6_m6A')).models['MG'].kind == 'mlp'


def test_rf_training_no_longer_needs_sklearn(monkeypatch):
    """`--train -c RF` goes to the GPU fitter, never to scikit-learn (which is blocked here): without a GPU the call fails in
    the device layer, not with the ImportError of the scikit-learn path."""
    from mcaller_amd import train_model
    block_sklearn(monkeypatch)
    called = {}

    def fake_fit(labs, sigs, grps, use_groups, device=None):
        called['n'] = len(labs)
        trees = fo.fit_forest(np.asarray(sigs), np.asarray([lab == 'm6A' for lab in labs], dtype=np.int64), np.arange(len(labs)), 1,
                              n_trees=3)
        return ['A', 'm6A'], np.full(5, 0.5), as_fit(trees, 7)

    monkeypatch.setattr(train_model, 'fit_rf_on_gpu', fake_fit)
    X, y = seven_features(60, 2)
    sig = {'general': {'A': [list(r) for r in X[y == 0]], 'm6A': [list(r) for r in X[y == 1]]}}
    grp = {'general': {'A': [str(i % 7) for i in range(int((y == 0).sum()))], 'm6A': [str(i % 7) for i in range(int((y == 1).sum()))]}}
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        train_model.train_classifier(sig, grp, d + '/m.npz', 'RF')
    assert called['n'] == 2 * min((y == 0).sum(), (y == 1).sum())
