"""The random-forest fit on the GPU (mc_forest_fit, k5_forest_fit) against its CPU restatement (tests/forest_fit_oracle.py): node
for node, bit for bit; the fitted forests scored by k3_forest; `--train -c RF` end to end."""
import contextlib
import io
import os
import pickle
import shutil

import numpy as np
import pytest

from tests import forest_fit_oracle as fo
from tests import helpers as H
from tests.helpers import block_sklearn

pytestmark = pytest.mark.gpu
FIELDS = ('left', 'right', 'feature', 'threshold', 'value', 'impurity', 'n_node_samples', 'weighted_n_node_samples')


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def data(n, d, seed, rounding=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * np.linspace(0.5, 3.0, d)
    X[:, -1] = 7.0 + 0.1 * rng.integers(0, 4, n)                     # (a read-quality-like column: few distinct values)
    if rounding is not None:
        X[:, :-1] = np.round(X[:, :-1], rounding)
    z = X[:, 0] - 0.7 * X[:, 1] + 0.3 * np.sin(3 * X[:, min(2, d - 1)])
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-2.0 * z))).astype(np.uint8)
    return X, y


def assert_same_forest(got, trees):
    """Device.forest_fit's arrays of one job == the oracle's list of trees, exactly."""
    off = got['tree_off']
    assert len(off) == len(trees) + 1
    for t, tr in enumerate(trees):
        a, b = off[t], off[t + 1]
        assert b - a == len(tr['left']), 'tree %d: %d nodes against %d' % (t, b - a, len(tr['left']))
        for f in FIELDS:
            g, w = np.asarray(got[f][a:b]), np.asarray(tr[f])
            assert g.shape == w.shape and (g.view(np.uint8) == w.astype(g.dtype).view(np.uint8)).all(), 'tree %d field %s' % (t, f)


def five_fold_jobs(n, seed):
    fold = np.random.default_rng(seed).integers(0, 5, n)
    rows = np.arange(n)
    return [(rows[fold != f], rows[fold == f]) for f in range(5)] + [(rows, np.zeros(0, np.int64))]


def test_five_folds_and_final_fit_in_one_call_equal_the_oracle(dev):
    X, y = data(2000, 7, 1)
    jobs = five_fold_jobs(len(y), 2)
    seeds = [(123 + 0x9E3779B97F4A7C15 * j) % (1 << 64) for j in range(6)]
    prm = dict(fo.REFERENCE, n_trees=12)
    got = dev.forest_fit(X, y, jobs, seeds=seeds, **prm)
    want = fo.fit_jobs(X, y, jobs, seeds, **prm)
    for j in range(6):
        assert_same_forest(got[j], want[j]['trees'])
        assert got[j]['val_correct'] == want[j]['val_correct'] and got[j]['n_val'] == len(jobs[j][1])
    assert got[0]['val_correct'] > 0.6 * got[0]['n_val']


@pytest.mark.parametrize('n,d,rounding,prm', [
    (5, 4, None, {}),                                     # five rows: trees whose root is a leaf
    (40, 4, 0, {}),                                       # heavy duplicates
    (600, 9, 1, {}),
    (3000, 7, None, dict(max_depth=16)),                  # deeper trees
    (3000, 4, 2, dict(max_features=2, min_samples_leaf=1, min_samples_split=2)),
    (800, 7, None, dict(bootstrap=False)),
    (20000, 7, None, dict(n_trees=3)),
])
def test_shapes_equal_the_oracle(dev, n, d, rounding, prm):
    X, y = data(n, d, n + d, rounding)
    rows = np.arange(n)
    jobs = [(rows[rows % 4 != 0], rows[rows % 4 == 0]) if n >= 8 else (rows, rows)]
    p = dict(fo.REFERENCE, n_trees=6)
    p.update(prm)
    got = dev.forest_fit(X, y, jobs, seeds=[77], **p)
    want = fo.fit_jobs(X, y, jobs, [77], **p)
    assert_same_forest(got[0], want[0]['trees'])
    assert got[0]['val_correct'] == want[0]['val_correct']
    if n == 5:
        assert any(len(t['left']) == 1 for t in want[0]['trees'])


def test_same_seed_same_forest_and_parameter_checks(dev):
    X, y = data(1500, 7, 3)
    jobs = five_fold_jobs(len(y), 4)
    a = dev.forest_fit(X, y, jobs, seed=9, n_trees=10)
    b = dev.forest_fit(X, y, jobs, seed=9, n_trees=10)
    for ga, gb in zip(a, b):
        for f in FIELDS + ('tree_off',):
            assert (np.asarray(ga[f]) == np.asarray(gb[f])).all()
        assert ga['val_correct'] == gb['val_correct']
    with pytest.raises(ValueError):
        dev.forest_fit(X[:, :3], y, jobs, seed=9)                # max_features=4 > 3 features, as scikit-learn refuses
    from mcaller_amd._lib import McError
    with pytest.raises(McError):
        dev.forest_fit(X, y, jobs, seed=9, max_depth=31)


def test_fitted_forest_scored_by_k3_forest_equals_the_oracle_and_sklearn(dev):
    from mcaller_amd.model_io import forest_from_arrays
    from mcaller_amd.train_model import as_sklearn_forest
    X, y = data(3000, 7, 5)
    rows = np.arange(len(y))
    got = dev.forest_fit(X, y, [(rows, rows[:0])], seeds=[5], **fo.REFERENCE)[0]
    trees = fo.fit_jobs(X, y, [(rows, rows[:0])], [5], **fo.REFERENCE)[0]['trees']
    assert_same_forest(got, trees)
    Xq, _ = data(4000, 7, 6)
    w = forest_from_arrays(got['tree_off'], got['left'], got['right'], got['feature'], got['threshold'], got['value'], 7)
    dev.set_classifier([w], np.zeros(256, dtype=np.uint8))
    p = dev.classifier_forward(Xq, np.zeros(len(Xq), dtype=np.uint8))
    _, want = fo.predict_proba(trees, Xq)
    assert (p == want).all()
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return
    rf = pickle.loads(pickle.dumps(as_sklearn_forest(dict(got, n_features=7), ['A', 'm6A'])))
    assert (rf.predict_proba(Xq)[:, 1] == want).all()


@pytest.mark.parametrize('with_sklearn', [True, False])
def test_train_rf_cli_then_score_with_the_written_file(tmp_path, monkeypatch, with_sklearn):
    """`mCaller --train -c RF` on labelled rows: the reference's lines, the model file (a pickle, or the neutral .npz without
    scikit-learn) holding the oracle's final forest; that forest, as a bare estimator file, then scores the eventalign file through
    `mCaller -c RF -d`: every record's probability is the oracle forest's."""
    if with_sklearn:
        pytest.importorskip('sklearn')
    else:
        block_sklearn(monkeypatch)
    from mcaller_amd import mCaller, train_model
    from mcaller_amd.load_mCaller_data import tsv2matrix
    from mcaller_amd.model_io import load_model_file
    td = H.testdata_paths(str(tmp_path))
    rows = str(tmp_path / 'training_rows.train')
    shutil.copy(os.path.join(H.GOLDEN, 'train', 'training_rows.train'), rows)
    model = str(tmp_path / 'model_RF_6_m6A.pkl')
    monkeypatch.setenv('MCALLER_SEED', '31')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '--train',
                      '--training_tsv', rows, '-c', 'RF', '-d', model])
    out = buf.getvalue()
    assert 'RF general model scores: ' in out and 'Cross validation accuracy: ' in out
    scores = [float(x) for x in out.split('RF general model scores: ')[1].split('\n')[0].split(',')]
    assert len(scores) == 5 and all(0.0 <= s <= 1.0 for s in scores)
    assert (open(model, 'rb').read(2) == b'PK') != with_sklearn
    # the oracle's six forests on the same rows, jobs and seeds
    sig, grp = tsv2matrix(rows, 'A')
    labs, sigs, grps = train_model.balanced_rows(sig['general'], grp['general'])
    classes, y, jobs, seeds = train_model.cv_jobs(labs, grps, bool(grp))
    X = np.asarray(sigs, dtype=np.float64)
    want = fo.fit_jobs(X, y, jobs, seeds, **fo.REFERENCE)
    assert scores == [w['val_correct'] / float(w['n_val']) for w in want[:5]]
    ms = load_model_file(model)
    w = ms.models['general']
    assert ms.twobase and w.kind == 'forest' and w.n_trees == 50 and w.n_in == 7 and w.classes == classes
    final = want[5]['trees']
    assert (w.tree_off == np.cumsum([0] + [len(t['left']) for t in final])).all()
    cat = lambda k: np.concatenate([t[k] for t in final])                       # noqa: E731
    base = np.repeat(w.tree_off[:-1], np.diff(w.tree_off))
    assert (w.left == np.where(cat('left') >= 0, cat('left') + base, -1)).all()
    assert (w.feature == cat('feature')).all() and (w.threshold == cat('threshold')).all() and (w.value == cat('value')).all()
    # the forest as a bare estimator file (the dict's key 'general' is no two-base sub-model): the calling run scores with it
    bare = str(tmp_path / ('bare_RF.pkl' if with_sklearn else 'bare_RF.npz'))
    if with_sklearn:
        with open(model, 'rb') as fh:
            est = pickle.load(fh)['general']
        assert (est.predict_proba(X)[:, 1] == fo.predict_proba(final, X)[1]).all()
        with open(bare, 'wb') as fh:
            pickle.dump(est, fh)
    else:
        z = np.load(model)
        np.savez(bare, **{k: z[k] for k in z.files if not k.startswith('__')})
    assert not load_model_file(bare).twobase
    with contextlib.redirect_stdout(io.StringIO()):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '-c', 'RF', '-d', bare])
    recs = [line.rstrip('\n').split('\t') for line in open(td['tsv'][:-4] + '.diffs.6')]
    assert len(recs) > 20
    Xr = np.array([[float(v) for v in r[4].split(',')] for r in recs])
    _, p = fo.predict_proba(final, Xr)
    assert [float(r[-1]) for r in recs] == [float(np.round(q, 2)) for q in p]
