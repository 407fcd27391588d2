"""The LR and NBC fits on the GPU (mc_lr_fit: k7_lr_fit; mc_nb_fit: k7_nb_fit) against their CPU restatements
(tests/lr_fit_oracle.py, tests/nb_fit_oracle.py); the fitted models scored by k3_simple; `--train -c LR|NBC` end to end with and
without scikit-learn."""
import contextlib
import io
import os
import pickle
import shutil

import numpy as np
import pytest

from oracle import clf_oracle
from tests import helpers as H
from tests import lr_fit_oracle as lo
from tests import nb_fit_oracle as no
from tests.helpers import block_sklearn, fit_data as data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def some_jobs(n, y):
    rows = np.arange(n)
    if n < 8:
        return [(rows, rows), (rows, np.zeros(0, np.int64))]
    jobs = [(rows[rows % 3 != 0], rows[rows % 3 == 0]), (rows, np.zeros(0, np.int64)), (rows[::-1][rows % 2 == 0], rows[rows % 2 == 1])]
    return [(tr, va) for tr, va in jobs if len(np.unique(y[tr])) == 2]


def assert_lr_matches(X, y, tr, va, got, want):
    Xt, yt = X[tr], y[tr]
    wg = np.concatenate([got['coef'], [got['intercept']]])
    ww = want['w']
    og, ow = lo.objective(Xt, yt, wg), lo.objective(Xt, yt, ww)
    assert abs(og - ow) <= 1e-9 * abs(ow), (og, ow)
    assert got['status'] == want['status']
    if lo.stopping_holds(Xt, yt, ww):
        assert lo.stopping_holds(Xt, yt, wg)
    scale = max(1.0, np.abs(ww).max())
    if got['n_iter'] == want['n_iter']:
        assert np.abs(wg - ww).max() <= 1e-9 * scale
    G = lo.gradient(Xt, yt, ww)
    edge = np.abs(np.abs(G) - 1.0) <= 1e-6
    assert ((wg == 0) == (ww == 0))[~edge].all()
    if len(va):
        diff = np.abs(got['val_dec'] - want['val_dec'])
        band = np.abs(want['val_dec']) <= diff + 1e-12
        assert ((got['val_dec'] > 0) == (want['val_dec'] > 0))[~band].all()
        assert abs(got['val_correct'] - want['val_correct']) <= band.sum()


@pytest.mark.parametrize('n,d,rounding', [(5, 1, None), (40, 4, 0), (600, 9, 1), (3000, 64, None), (3000, 3, 0), (9244, 7, None),
                                          (50000, 7, None)])
def test_lr_fits_equal_the_oracle_and_repeat_bit_for_bit(dev, n, d, rounding):
    X, y = data(n, d, n + d, rounding)
    if n == 5:
        y = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    jobs = some_jobs(n, y)
    seeds = [1234567 + 17 * j for j in range(len(jobs))]
    got = dev.lr_fit(X, y, jobs, seeds)
    again = dev.lr_fit(X, y, jobs, seeds)
    for a, b in zip(got, again):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for (tr, va), s, fit in zip(jobs, seeds, got):
        assert fit['n_val'] == len(va) and fit['n_iter'] >= 1
        assert_lr_matches(X, y, tr, va, fit, lo.solve_job(X, y, tr, va, s))


def test_lr_separable_rows_stop_at_the_iteration_cap(dev):
    """Separable rows need ~10 Newton iterations (the L1 term keeps w finite); a cap of 4 stops them: status 1, as scikit-learn's
    ConvergenceWarning, with the oracle's w."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 3)) * 100.0
    y = (X[:, 0] > 0).astype(np.uint8)
    X[:, 0] += np.where(y == 1, 50.0, -50.0)
    rows = np.arange(300)
    got = dev.lr_fit(X, y, [(rows, rows[:50])], [77], max_iter=4)[0]
    want = lo.solve_job(X, y, rows, rows[:50], 77, max_iter=4)
    assert want['status'] == 1 and got['status'] == 1 and got['n_iter'] == 4
    assert_lr_matches(X, y, rows, rows[:50], got, want)


@pytest.mark.parametrize('n,d,rounding', [(5, 1, None), (40, 4, 0), (600, 9, 1), (3000, 64, None), (9244, 7, None), (50000, 7, None)])
def test_nb_fits_equal_the_oracle(dev, n, d, rounding):
    X, y = data(n, d, n + d + 1, rounding)
    if n == 5:
        y = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    jobs = some_jobs(n, y)
    got = dev.nb_fit(X, y, jobs)
    again = dev.nb_fit(X, y, jobs)
    for (tr, va), fit, fit2 in zip(jobs, got, again):
        want = no.fit_job(X, y, tr, va)
        for k in ('theta', 'var'):
            assert np.abs(fit[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
            assert np.array_equal(fit[k], fit2[k])
        assert abs(fit['epsilon'] - want['epsilon']) <= 1e-12 * want['epsilon']
        assert (fit['class_count'] == want['class_count']).all()
        band = (np.abs(want['val_gap']) < 1e-9 * (1 + np.abs(no.joint_log_likelihood(want, X[va])).max(axis=1))).sum() if len(va) else 0
        assert abs(fit['val_correct'] - want['val_correct']) <= band


def cli_like(n, d, seed):
    from mcaller_amd import train_model
    X, y = data(n, d, seed)
    labs = list(np.array(['A', 'm6A'])[y])
    grps = ['g%d' % (i % 41) for i in range(n)]
    return X, y, labs, grps, train_model


def test_fitted_models_scored_by_k3_simple_equal_the_estimators(dev, monkeypatch):
    from mcaller_amd.model_io import GaussianNBWeights, LogisticWeights
    X, y, labs, grps, tm = cli_like(2500, 7, 4)
    monkeypatch.setenv('MCALLER_SEED', '77')
    Xq, _ = data(4000, 7, 6)
    zeros = np.zeros(len(Xq), dtype=np.uint8)
    classes, scores, lr = tm.fit_lr_on_gpu(labs, X.tolist(), grps, True, device=dev)
    _, _, nb = tm.fit_nb_on_gpu(labs, X.tolist(), grps, True, device=dev)
    wl = LogisticWeights(lr['coef'], [lr['intercept']], classes)
    wn = GaussianNBWeights(nb['theta'], nb['var'], nb['class_prior'], classes)
    dev.set_classifier([wl], np.zeros(256, dtype=np.uint8))
    pl = dev.classifier_forward(Xq, zeros)
    assert np.abs(pl - clf_oracle.logistic_proba(wl.coef, wl.intercept, Xq)).max() <= 1e-12
    dev.set_classifier([wn], np.zeros(256, dtype=np.uint8))
    pn = dev.classifier_forward(Xq, zeros)
    assert np.abs(pn - clf_oracle.gnb_proba(wn.theta, wn.var, wn.prior, Xq)).max() <= 1e-12
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return
    est = pickle.loads(pickle.dumps(tm.as_sklearn_logistic(lr, classes)))
    assert np.abs(est.predict_proba(Xq)[:, 1] - pl).max() <= 1e-12
    est = pickle.loads(pickle.dumps(tm.as_sklearn_gnb(nb, classes)))
    assert np.abs(est.predict_proba(Xq)[:, 1] - pn).max() <= 1e-12


def test_bad_parameters_raise_and_never_fault(dev):
    from mcaller_amd import _lib
    import ctypes as C
    X, y = data(100, 4, 1)
    rows = np.arange(100)
    jobs = [(rows, rows[:10])]
    for fit in (lambda *a: dev.lr_fit(*a, [5]), lambda *a: dev.nb_fit(*a)):
        with pytest.raises(ValueError):
            fit(X[:, :0], y, jobs)                                     # n_in 0
        with pytest.raises(ValueError):
            fit(np.zeros((100, 65)), y, jobs)                          # n_in 65
        bad = X.copy()
        bad[3, 1] = np.nan
        with pytest.raises(ValueError):
            fit(bad, y, jobs)
        with pytest.raises(ValueError):
            fit(X, np.where(y == 1, 2, 0).astype(np.uint8), jobs)
        with pytest.raises(ValueError):
            fit(X, y, [(np.array([0, 200]), rows[:5])])
        with pytest.raises(ValueError):
            fit(X, y, [(rows, np.array([-1]))])
        with pytest.raises(ValueError):
            fit(X, y, [(rows[y == 0], rows[:5])])                      # one class
    with pytest.raises(ValueError):
        dev.nb_fit(np.ones((10, 3)), np.array([0, 1] * 5, np.uint8), [(np.arange(10), np.arange(3))])   # epsilon_ = 0
    with pytest.raises(ValueError):
        dev.lr_fit(X, y, jobs, [5], C=0.0)
    L = _lib.lib()
    z = np.zeros(256)
    prm = _lib.LrParams(1.0, 1e-4, 100, 0)
    one_class = rows[y == 0].astype(np.int32)
    rc = L.mc_lr_fit(dev._ctx, C.byref(prm), _lib._ptr(np.ascontiguousarray(X)), _lib._ptr(y), 100, 4, 1,
                     _lib._ptr(np.array([0, len(one_class)], np.int64)), _lib._ptr(one_class), _lib._ptr(np.zeros(2, np.int64)),
                     _lib._ptr(np.zeros(1, np.int32)), _lib._ptr(np.array([5], np.uint32)), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z),
                     _lib._ptr(z), _lib._ptr(z), _lib._ptr(z))
    assert rc == -12 and b'one class' in L.mc_last_error()
    nprm = _lib.NbParams(1e-9)
    rc = L.mc_nb_fit(dev._ctx, C.byref(nprm), _lib._ptr(np.ascontiguousarray(X)), _lib._ptr(y), 100, 65, 1,
                     _lib._ptr(np.array([0, 100], np.int64)), _lib._ptr(rows.astype(np.int32)), _lib._ptr(np.zeros(2, np.int64)),
                     _lib._ptr(np.zeros(1, np.int32)), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z))
    assert rc == -12 and b'n_in 65' in L.mc_last_error()
    ok = dev.lr_fit(X, y, jobs, [5])[0]                                # (the context still works)
    assert ok['n_iter'] >= 1


@pytest.mark.parametrize('with_sklearn', [True, False])
@pytest.mark.parametrize('clf', ['LR', 'NBC'])
def test_train_cli_then_score_with_the_written_file(tmp_path, monkeypatch, with_sklearn, clf):
    """`mCaller --train -c LR|NBC` on labelled rows: the reference's lines, the model file (a pickle, or the neutral .npz without
    scikit-learn, which failed with ImportError before the GPU fits), CV scores equal to the oracle's outside the band; the model,
    as a bare estimator file, then scores the eventalign file through `mCaller -c LR|NBC -d` with the oracle's probabilities."""
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
    model = str(tmp_path / ('model_%s_6_m6A.pkl' % clf))
    monkeypatch.setenv('MCALLER_SEED', '31')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '--train',
                      '--training_tsv', rows, '-c', clf, '-d', model])
    out = buf.getvalue()
    sig, grp = tsv2matrix(rows, 'A')
    labs, sigs, grps = train_model.balanced_rows(sig['general'], grp['general'])
    lines = out.split('\n')
    k = lines.index(str(labs[:10]))
    assert lines[k + 1] == str(sigs[:10]) and lines[k + 2] == str(grps[:10])
    head = '%s general model scores: ' % clf
    assert lines[k + 3].startswith(head) and lines[k + 4].startswith('Cross validation accuracy: ')
    scores = [float(x) for x in lines[k + 3].split(head)[1].split(',')]
    assert (open(model, 'rb').read(2) == b'PK') != with_sklearn
    classes, y, jobs, seeds = train_model.cv_jobs(labs, grps, bool(grp))
    X = np.asarray(sigs, dtype=np.float64)
    for f, (tr, va) in enumerate(jobs[:5]):
        if len(np.unique(y[tr])) < 2:
            assert np.isnan(scores[f]) if clf == 'LR' else scores[f] == np.mean(y[va] == y[tr[0]])
            continue
        if clf == 'LR':
            w = lo.solve_job(X, y, tr, va, train_model.platt_seed(seeds[f]))
            band = (np.abs(w['val_dec']) < 1e-6).sum()
        else:
            w = no.fit_job(X, y, tr, va)
            band = (np.abs(w['val_gap']) < 1e-9).sum()
        assert abs(round(scores[f] * len(va)) - w['val_correct']) <= band
    ms = load_model_file(model)
    wt = ms.models['general']
    assert ms.twobase and wt.kind == ('logistic' if clf == 'LR' else 'gnb') and wt.n_in == 7 and wt.classes == classes
    if clf == 'LR':
        want = lo.solve_job(X, y, np.arange(len(y)), np.zeros(0, np.int64), train_model.platt_seed(seeds[5]))['w']
        assert abs(lo.objective(X, y, wt.params()) - lo.objective(X, y, want)) <= 1e-9 * lo.objective(X, y, want)
    else:
        want = no.fit(X, y)
        assert np.abs(wt.theta - want['theta']).max() <= 1e-12 * np.abs(want['theta']).max()
        assert np.abs(wt.var - want['var']).max() <= 1e-12 * np.abs(want['var']).max()
    proba = (lambda Z: clf_oracle.logistic_proba(wt.coef, wt.intercept, Z)) if clf == 'LR' else \
        (lambda Z: clf_oracle.gnb_proba(wt.theta, wt.var, wt.prior, Z))
    bare = str(tmp_path / ('bare_%s.pkl' % clf if with_sklearn else 'bare_%s.npz' % clf))
    if with_sklearn:
        with open(model, 'rb') as fh:
            est = pickle.load(fh)['general']
        assert np.abs(est.predict_proba(X)[:, 1] - proba(X)).max() <= 1e-12
        with open(bare, 'wb') as fh:
            pickle.dump(est, fh)
    else:
        z = np.load(model)
        np.savez(bare, **{k: z[k] for k in z.files if not k.startswith('__')})
    assert not load_model_file(bare).twobase
    with contextlib.redirect_stdout(io.StringIO()):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '-c', clf, '-d', bare])
    recs = [line.rstrip('\n').split('\t') for line in open(td['tsv'][:-4] + '.diffs.6')]
    assert len(recs) > 20
    Xr = np.array([[float(v) for v in r[4].split(',')] for r in recs])
    p = proba(Xr)
    assert [float(r[-1]) for r in recs] == [float(np.round(q, 2)) for q in p]
