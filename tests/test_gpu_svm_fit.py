"""The RBF SVC fit on the GPU (mc_svm_fit: k6_svm_fit, k6_svm_val, k6_svm_sigmoid) against its CPU restatement
(tests/svm_fit_oracle.py); the fitted model scored by k3_svm; `--train -c SVM` end to end with and without scikit-learn."""
import contextlib
import io
import os
import pickle
import shutil

import numpy as np
import pytest

from tests import helpers as H
from tests import svm_fit_oracle as so
from tests import svm_oracle
from tests.helpers import block_sklearn, fit_data as data

pytestmark = pytest.mark.gpu
BAND = 5e-3


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def assert_solve_matches(X, y, train, val, gamma, got, want):
    ys = np.where(y[train] == y[train[0]], 1.0, -1.0)
    assert got['status'] == 0 and got['n_iter'] > 0
    assert so.kkt_violation(X[train], ys, got['alpha'], gamma) <= 1e-3
    sg, sw = got['alpha'] > 0, want['alpha'] > 0
    og = so.dual_objective(X[train][sg], (ys * got['alpha'])[sg], gamma)
    ow = so.dual_objective(X[train][sw], (ys * want['alpha'])[sw], gamma)
    assert abs(og - ow) <= 1e-6 * abs(ow)
    if len(val):
        assert np.abs(got['val_dec'] - want['val_dec']).max() <= BAND
        band = np.abs(want['val_dec']) < BAND
        assert ((got['val_dec'] > 0) == (want['val_dec'] > 0))[~band].all()
        assert abs(got['val_correct'] - want['val_correct']) <= band.sum()


@pytest.mark.parametrize('n,d,rounding', [(5, 1, None), (40, 4, 0), (600, 9, 1), (3000, 7, None), (3000, 3, 0), (9244, 7, None),
                                          (20000, 7, None)])
def test_solves_equal_the_oracle(dev, n, d, rounding):
    X, y = data(n, d, n + d, rounding)
    if n == 5:
        y = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    rows = np.arange(n)
    if n >= 20000:                                                 # one job
        jobs = [(so.grouped(rows[rows % 4 != 0], y, 0), rows[rows % 4 == 0])]
    else:                                                          # classes_[0] first, and classes_[1] first (a Platt fold)
        tr, va = (rows, rows) if n < 8 else (rows[rows % 3 != 0], rows[rows % 3 == 0])
        jobs = [(so.grouped(tr, y, 0), va), (so.grouped(tr, y, 1), va)]
    gammas = [so.gamma_of(X[tr]) for tr, _ in jobs]
    got = dev.svm_fit(X, y, jobs, gammas)
    for (tr, va), g, fit in zip(jobs, gammas, got):
        assert_solve_matches(X, y, tr, va, g, fit, so.solve_job(X, y, tr, va, g))


def test_zero_variance_gives_gamma_one_and_duplicates_solve(dev):
    X = np.full((64, 3), 1.5)
    X[::2, 0] = 1.5                                               # (every row the same point)
    y = (np.arange(64) % 2).astype(np.uint8)
    assert so.gamma_of(X) == 1.0
    rows = np.arange(64)
    tr = so.grouped(rows, y, 0)
    got = dev.svm_fit(X, y, [(tr, rows)], [1.0])[0]
    assert_solve_matches(X, y, tr, rows, 1.0, got, so.solve_job(X, y, tr, rows, 1.0))


def cli_like(n, d, seed):
    from mcaller_amd import train_model
    X, y = data(n, d, seed)
    labs = list(np.array(['A', 'm6A'])[y])
    grps = ['g%d' % (i % 41) for i in range(n)]
    return X, y, labs, grps, train_model


def test_a_sub_model_fit_equals_the_oracle_and_repeats_bit_for_bit(dev, monkeypatch):
    X, y, labs, grps, tm = cli_like(1200, 7, 3)
    monkeypatch.setenv('MCALLER_SEED', '1234')
    classes, scores, fit = tm.fit_svm_on_gpu(labs, X.tolist(), grps, True, device=dev)
    _, scores2, fit2 = tm.fit_svm_on_gpu(labs, X.tolist(), grps, True, device=dev)
    assert (scores == scores2).all()
    for k in fit:
        assert np.array_equal(np.asarray(fit[k]), np.asarray(fit2[k])), k
    _, yy, jobs, seeds = tm.cv_jobs(labs, grps, True)
    want = so.fit_submodel(X, y, jobs, seeds[5])
    plan = tm.svm_plan(X, y, jobs, seeds[5])
    assert (plan['perm'] == want['perm']).all() and plan['gammas'][:5] == want['gammas'][:5]
    for f, (tr, va) in enumerate(jobs[:5]):
        band = (np.abs(want['cv'][f]['val_dec']) < BAND).sum()
        assert abs(scores[f] * len(va) - want['cv'][f]['val_correct']) <= band
    # the Platt step: the device's own held-out decision values through the oracle's sigmoid_train
    fits = dev.svm_fit(X, y, plan['device'], plan['gammas'])
    dec = np.zeros(len(y))
    for job, held, const in plan['platt']:
        dec[held] = fits[job]['val_dec'] if job is not None else const
    assert np.abs(dec - want['platt_dec']).max() <= BAND
    A, B = so.sigmoid_train(dec, np.where(y[plan['order']] == 0, 1.0, -1.0))
    assert abs(fit['probA'] - A) <= 1e-12 * abs(A) and abs(fit['probB'] - B) <= 1e-12 * abs(B)
    dA, dB = dev.svm_sigmoid_train(dec, y[plan['order']])
    assert (dA, dB) == (fit['probA'], fit['probB'])
    ys = np.where(y[plan['order']] == 0, 1.0, -1.0)
    fin = fits[plan['final']]
    assert so.kkt_violation(X[plan['order']], ys, fin['alpha'], plan['gamma']) <= 1e-3
    assert (fit['support'] == plan['order'][fin['alpha'] > 0]).all() and fit['n_support'].sum() == len(fit['support'])


def test_the_fitted_model_scored_by_k3_svm_equals_the_oracle_and_sklearn(dev, monkeypatch):
    from mcaller_amd.model_io import SVMWeights
    X, y, labs, grps, tm = cli_like(2500, 7, 4)
    monkeypatch.setenv('MCALLER_SEED', '77')
    classes, scores, fit = tm.fit_svm_on_gpu(labs, X.tolist(), grps, True, device=dev)
    w = SVMWeights(fit['sv'], fit['dual_coef'], fit['gamma'], fit['intercept'], fit['probA'], fit['probB'], classes)
    Xq, _ = data(4000, 7, 6)
    dev.set_classifier([w], np.zeros(256, dtype=np.uint8))
    p = dev.classifier_forward(Xq, np.zeros(len(Xq), dtype=np.uint8))
    want = svm_oracle.proba(w, Xq)
    assert np.abs(p - want).max() <= 1e-12
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return
    est = pickle.loads(pickle.dumps(tm.as_sklearn_svc(fit, classes)))
    assert np.abs(est.predict_proba(Xq)[:, 1] - p).max() <= 1e-12


def test_bad_parameters_raise_and_never_fault(dev):
    from mcaller_amd._lib import McError
    X, y = data(100, 4, 1)
    rows = np.arange(100)
    jobs = [(so.grouped(rows, y, 0), rows[:10])]
    with pytest.raises(ValueError):
        dev.svm_fit(X, y, [(rows[y == 0], rows[:5])], [0.5])          # one class
    with pytest.raises(ValueError):
        dev.svm_fit(X, y, jobs, [0.0])
    with pytest.raises(ValueError):
        dev.svm_fit(X, y, jobs, [0.5], C=0.0)
    with pytest.raises(ValueError):
        dev.svm_fit(np.zeros((100, 65)), y, jobs, [0.5])
    with pytest.raises(ValueError):
        dev.svm_fit(X, y, [(np.array([0, 200]), rows[:5])], [0.5])
    with pytest.raises(ValueError):
        dev.svm_sigmoid_train(np.array([np.nan, 1.0]), np.array([0, 1]))
    from mcaller_amd import _lib
    import ctypes as C
    prm = _lib.SvmParams(-1.0, 1e-3, 0)
    L = _lib.lib()
    z = np.zeros(8)
    rc = L.mc_svm_fit(dev._ctx, C.byref(prm), _lib._ptr(np.ascontiguousarray(X)), _lib._ptr(y), 100, 4, 1,
                      _lib._ptr(np.array([0, 100], np.int64)), _lib._ptr(np.arange(100, dtype=np.int32)), _lib._ptr(np.zeros(2, np.int64)),
                      _lib._ptr(np.zeros(1, np.int32)), _lib._ptr(np.array([0.5])), _lib._ptr(np.zeros(100)), _lib._ptr(z), _lib._ptr(z),
                      _lib._ptr(z), _lib._ptr(z), _lib._ptr(z))
    assert rc == -12 and b'C must be' in L.mc_last_error()
    with pytest.raises(McError):                                      # (the C ABI's own check: no values)
        _lib.check(L.mc_svm_sigmoid_train(dev._ctx, _lib._ptr(z), _lib._ptr(np.zeros(8, np.uint8)), 0, C.byref(C.c_double()),
                                          C.byref(C.c_double())))
    capped = dev.svm_fit(X, y, jobs, [so.gamma_of(X)], max_iter=3)[0]
    assert capped['status'] == 1 and capped['n_iter'] == 3


@pytest.mark.parametrize('with_sklearn', [True, False])
def test_train_svm_cli_then_score_with_the_written_file(tmp_path, monkeypatch, with_sklearn):
    """`mCaller --train -c SVM` on labelled rows: the reference's lines, the model file (a pickle, or the neutral .npz without
    scikit-learn, which failed with ImportError before the GPU fit), CV scores equal to the oracle's outside the band; the model,
    as a bare estimator file, then scores the eventalign file through `mCaller -c SVM -d` with the oracle's probabilities."""
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
    model = str(tmp_path / 'model_SVM_6_m6A.pkl')
    monkeypatch.setenv('MCALLER_SEED', '31')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '--train',
                      '--training_tsv', rows, '-c', 'SVM', '-d', model])
    out = buf.getvalue()
    sig, grp = tsv2matrix(rows, 'A')
    labs, sigs, grps = train_model.balanced_rows(sig['general'], grp['general'])
    lines = out.split('\n')
    k = lines.index(str(labs[:10]))
    assert lines[k + 1] == str(sigs[:10]) and lines[k + 2] == str(grps[:10])
    assert lines[k + 3].startswith('SVM general model scores: ') and lines[k + 4].startswith('Cross validation accuracy: ')
    scores = [float(x) for x in lines[k + 3].split('SVM general model scores: ')[1].split(',')]
    assert (open(model, 'rb').read(2) == b'PK') != with_sklearn
    classes, y, jobs, seeds = train_model.cv_jobs(labs, grps, bool(grp))
    X = np.asarray(sigs, dtype=np.float64)
    want = so.fit_submodel(X, y, jobs, seeds[5])
    for f, (tr, va) in enumerate(jobs[:5]):
        w = want['cv'][f]
        if w is None:
            assert np.isnan(scores[f])
            continue
        band = (np.abs(w['val_dec']) < BAND).sum()
        assert abs(scores[f] * len(va) - w['val_correct']) <= band
    ms = load_model_file(model)
    wt = ms.models['general']
    assert ms.twobase and wt.kind == 'svm' and wt.n_in == 7 and wt.classes == classes
    assert wt.gamma == want['fit']['gamma'] and abs(wt.intercept - want['fit']['intercept']) <= BAND
    bare = str(tmp_path / ('bare_SVM.pkl' if with_sklearn else 'bare_SVM.npz'))
    if with_sklearn:
        with open(model, 'rb') as fh:
            est = pickle.load(fh)['general']
        assert np.abs(est.predict_proba(X)[:, 1] - svm_oracle.proba(wt, X)).max() <= 1e-12
        with open(bare, 'wb') as fh:
            pickle.dump(est, fh)
    else:
        z = np.load(model)
        np.savez(bare, **{k: z[k] for k in z.files if not k.startswith('__')})
    assert not load_model_file(bare).twobase
    with contextlib.redirect_stdout(io.StringIO()):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '-c', 'SVM', '-d', bare])
    recs = [line.rstrip('\n').split('\t') for line in open(td['tsv'][:-4] + '.diffs.6')]
    assert len(recs) > 20
    Xr = np.array([[float(v) for v in r[4].split(',')] for r in recs])
    p = svm_oracle.proba(wt, Xr)
    assert [float(r[-1]) for r in recs] == [float(np.round(q, 2)) for q in p]
