"""The `--train -c LR` / `-c NBC` fits' CPU restatements (tests/lr_fit_oracle.py, tests/nb_fit_oracle.py) against scikit-learn, the
host side of the fits (train_model.fit_lr_on_gpu / fit_nb_on_gpu on a stand-in device that runs the oracles), and the writers and
loader of the fitted models.  No GPU: the device is held to the oracles in tests/test_gpu_simple_fit.py."""
import warnings

import numpy as np
import pytest

from oracle import clf_oracle
from tests import lr_fit_oracle as lo
from tests import nb_fit_oracle as no
from tests.helpers import block_sklearn


def data(n, d, seed, rounding=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * np.linspace(0.5, 3.0, d)
    if d > 1:
        X[:, -1] = 7.0 + 0.1 * rng.integers(0, 4, n)
    if rounding is not None:
        X = np.round(X, rounding)
    z = X[:, 0] - 0.7 * X[:, min(1, d - 1)]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-2.0 * z))).astype(np.int64)
    return X, y


def lr_case(name):
    if name == 'config5':
        return data(9244, 7, 1)
    if name.startswith('rows'):
        n = int(name[4:])
        X, _ = data(n, 3, n)
        return X, np.arange(n) % 2
    if name == 'd1':
        return data(400, 1, 2)
    if name == 'd64':
        return data(600, 64, 3)
    if name == 'constant':
        X, y = data(500, 4, 4)
        X[:, 1] = 2.5                                             # collinear with the bias
        return X, y
    if name == 'zero':
        X, y = data(500, 4, 5)
        X[:, 2] = 0.0
        return X, y
    if name == 'ties':
        return data(800, 5, 6, rounding=0)
    if name == 'separable':
        rng = np.random.default_rng(5)
        X = rng.normal(size=(300, 3)) * 100.0
        y = (X[:, 0] > 0).astype(np.int64)
        X[:, 0] += np.where(y == 1, 50.0, -50.0)
        return X, y
    raise KeyError(name)


LR_CASES = ['config5', 'rows2', 'rows3', 'rows5', 'rows10', 'd1', 'd64', 'constant', 'zero', 'ties', 'separable']


@pytest.mark.parametrize('name', LR_CASES)
@pytest.mark.parametrize('r', [0, 7])
def test_lr_oracle_equals_liblinear(name, r):
    sk = pytest.importorskip('sklearn.linear_model')
    from sklearn.exceptions import ConvergenceWarning
    X, y = lr_case(name)
    o = lo.liblinear_order(y)
    X, y = X[o], y[o]
    max_iter = 4 if name == 'separable' else 100                   # (separable rows need ~10: the cap stops them)
    seed = np.random.RandomState(r).randint(np.iinfo('i').max)
    got = lo.solve(X, y, seed, max_iter=max_iter)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', ConvergenceWarning)
        m = sk.LogisticRegression(solver='liblinear', penalty='l1', random_state=r, max_iter=max_iter).fit(X, y)
    want = np.concatenate([m.coef_[0], m.intercept_])
    assert got['n_iter'] == int(m.n_iter_[0])
    assert got['status'] == (1 if int(m.n_iter_[0]) >= max_iter else 0)
    assert np.abs(got['w'] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if name == 'separable':
        assert got['status'] == 1
    if name == 'zero':
        assert got['w'][2] == 0.0


@pytest.mark.parametrize('name', ['config5', 'rows5', 'd1', 'd64', 'constant', 'zero', 'ties'])
def test_nb_oracle_equals_gaussian_nb(name):
    nb = pytest.importorskip('sklearn.naive_bayes')
    X, y = lr_case(name)
    got = no.fit(X, y)
    m = nb.GaussianNB().fit(X, y)
    for k, a in (('theta', m.theta_), ('var', m.var_)):
        assert np.abs(got[k] - a).max() <= 1e-13 * np.abs(a).max(), k
    assert abs(got['epsilon'] - m.epsilon_) <= 1e-13 * m.epsilon_
    assert (got['class_count'] == m.class_count_).all() and (got['class_prior'] == m.class_prior_).all()
    assert (no.predict(got, X) == m.predict(X)).all()


class OracleDevice(object):
    """Device.lr_fit / nb_fit answered by the oracles (the host code around them is what is tested here)."""

    def lr_fit(self, X, y, jobs, seeds, C=1.0, tol=1e-4, max_iter=100):
        out = []
        for (tr, va), s in zip(jobs, seeds):
            assert len(np.unique(y[tr])) == 2 and 0 <= s < 2 ** 31 - 1
            r = lo.solve_job(X, y, tr, va, s, C=C, tol=tol, max_iter=max_iter)
            out.append(dict(coef=r['w'][:-1], intercept=float(r['w'][-1]), n_iter=r['n_iter'], status=r['status'], val_dec=r['val_dec'],
                            val_correct=r['val_correct'], n_val=len(va)))
        return out

    def nb_fit(self, X, y, jobs, var_smoothing=1e-9):
        out = []
        for tr, va in jobs:
            assert len(np.unique(y[tr])) == 2
            r = no.fit_job(X, y, tr, va, var_smoothing)
            out.append(dict(theta=r['theta'], var=r['var'], epsilon=r['epsilon'], class_count=r['class_count'].astype(np.int64),
                            val_correct=r['val_correct'], n_val=len(va)))
        return out


def cli_like(n, seed, one_class_fold=False):
    X, y = data(n, 7, seed)
    grps = ['g%d' % (i % 23) for i in range(n)]
    if one_class_fold:                                            # every row of class 0 in one group: its fold trains on class 1 alone
        grps = ['g%d' % (i % 23) if y[i] == 1 else 'zero' for i in range(n)]
    return X, y, list(np.array(['A', 'm6A'])[y]), grps


@pytest.mark.parametrize('clf', ['LR', 'NBC'])
@pytest.mark.parametrize('one_class_fold', [False, True])
def test_fold_scores_equal_cross_val_score(clf, one_class_fold, monkeypatch):
    pytest.importorskip('sklearn')
    from sklearn.linear_model import LogisticRegression
    from sklearn.model_selection import GroupKFold, cross_val_score
    from sklearn.naive_bayes import GaussianNB
    from mcaller_amd import train_model as tm
    X, y, labs, grps = cli_like(1500 if not one_class_fold else 400, 3, one_class_fold)
    if one_class_fold:                                            # (a group larger than the others takes a fold of its own)
        keep = [i for i in range(len(y)) if y[i] == 1 or i % 4 == 0]
        X, y, labs, grps = X[keep], y[keep], [labs[i] for i in keep], [grps[i] for i in keep]
    monkeypatch.setenv('MCALLER_SEED', '99')
    fit = tm.fit_lr_on_gpu if clf == 'LR' else tm.fit_nb_on_gpu
    classes, scores, final = fit(labs, X.tolist(), grps, True, device=OracleDevice())
    _, yy, jobs, seeds = tm.cv_jobs(labs, grps, True)
    one = [len(np.unique(yy[tr])) < 2 for tr, _ in jobs[:5]]
    assert any(one) == one_class_fold
    for f, (tr, va) in enumerate(jobs[:5]):
        if clf == 'LR' and one[f]:
            assert np.isnan(scores[f])
            continue
        if clf == 'LR':
            seed = tm.platt_seed(seeds[f])
            o = lo.liblinear_order(yy[tr])
            want = lo.solve(X[tr][o], yy[tr][o], seed)['w']
            dec = lo.decision(X[va], want)
            band = np.abs(dec) < 1e-9
            pred = (dec > 0).astype(int)
        else:
            m = GaussianNB().fit(X[tr], np.asarray(labs)[tr])
            pred = (m.predict(X[va]) == classes[1]).astype(int)
            band = np.zeros(len(va), bool)
        right = (pred == yy[va])
        assert abs(round(scores[f] * len(va)) - right.sum()) <= band.sum()
    if clf == 'NBC':                                              # cross_val_score itself, one-class folds included
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = cross_val_score(GaussianNB(), X, labs, cv=GroupKFold(n_splits=5), groups=grps)
        assert np.abs(scores - want).max() <= 1e-12
    elif not one_class_fold:                                      # (liblinear's own seeds differ from ours: outside the band only)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = cross_val_score(LogisticRegression(solver='liblinear', penalty='l1'), X, labs, cv=GroupKFold(n_splits=5), groups=grps)
        assert np.abs(scores - want).max() <= 2.0 / min(len(va) for _, va in jobs[:5])


def final_fits():
    from mcaller_amd import train_model as tm
    X, y, labs, grps = cli_like(900, 8)
    dev = OracleDevice()
    classes, _, lr = tm.fit_lr_on_gpu(labs, X.tolist(), grps, True, device=dev)
    _, _, nb = tm.fit_nb_on_gpu(labs, X.tolist(), grps, True, device=dev)
    return X, classes, lr, nb


def test_estimators_predict_what_the_weights_score():
    pytest.importorskip('sklearn')
    import pickle
    from mcaller_amd import train_model as tm
    from mcaller_amd.model_io import GaussianNBWeights, LogisticWeights
    X, classes, lr, nb = final_fits()
    Xq, _ = data(3000, 7, 11)
    est = pickle.loads(pickle.dumps(tm.as_sklearn_logistic(lr, classes)))
    w = LogisticWeights(lr['coef'], [lr['intercept']], classes)
    assert list(est.classes_) == classes and est.n_iter_.dtype == np.int32 and est.coef_.shape == (1, 7)
    assert np.abs(est.predict_proba(Xq)[:, 1] - clf_oracle.logistic_proba(w.coef, w.intercept, Xq)).max() <= 1e-12
    est = pickle.loads(pickle.dumps(tm.as_sklearn_gnb(nb, classes)))
    g = GaussianNBWeights(nb['theta'], nb['var'], nb['class_prior'], classes)
    assert est.epsilon_ == nb['epsilon'] and (est.class_count_ == nb['class_count']).all()
    assert np.abs(est.predict_proba(Xq)[:, 1] - clf_oracle.gnb_proba(g.theta, g.var, g.prior, Xq)).max() <= 1e-12


def test_npz_round_trips_without_sklearn(tmp_path, monkeypatch):
    from mcaller_amd import train_model as tm
    from mcaller_amd.model_io import load_model_file, shipped_model
    X, classes, lr, nb = final_fits()
    block_sklearn(monkeypatch)
    for clf, fit in (('LR', lr), ('NBC', nb)):
        path = str(tmp_path / ('m_%s.pkl' % clf))
        tm.write_models({'general': fit}, {'general': classes}, {'general': len(X)}, path, clf)
        assert open(path, 'rb').read(2) == b'PK'
        ms = load_model_file(path)
        w = ms.models['general']
        assert ms.twobase and w.classes == classes and w.n_in == 7
        if clf == 'LR':
            assert w.kind == 'logistic' and (w.coef == lr['coef']).all() and w.intercept == lr['intercept']
        else:
            assert w.kind == 'gnb' and (w.theta == nb['theta']).all() and (w.var == nb['var']).all()
            assert (w.prior == nb['class_prior']).all()
    assert load_model_file(shipped_model('r95_twobase_model_NN_6_m6A')).models['MG'].kind == 'mlp'


@pytest.mark.parametrize('clf', ['LR', 'NBC'])
def test_lr_and_nbc_training_no_longer_need_sklearn(clf, monkeypatch, tmp_path):
    """`--train -c LR|NBC` goes to the GPU fitters, never to scikit-learn (blocked here; the call raised ImportError before)."""
    from mcaller_amd import train_model
    block_sklearn(monkeypatch)
    called = {}
    real = train_model.fit_lr_on_gpu if clf == 'LR' else train_model.fit_nb_on_gpu

    def fake_fit(labs, sigs, grps, use_groups, device=None):
        called['n'] = len(labs)
        return real(labs, sigs, grps, use_groups, device=OracleDevice())

    monkeypatch.setattr(train_model, 'fit_lr_on_gpu' if clf == 'LR' else 'fit_nb_on_gpu', fake_fit)
    X, y = data(120, 7, 2)
    sig = {'general': {'A': [list(r) for r in X[y == 0]], 'm6A': [list(r) for r in X[y == 1]]}}
    grp = {'general': {'A': [str(i % 7) for i in range(int((y == 0).sum()))], 'm6A': [str(i % 7) for i in range(int((y == 1).sum()))]}}
    train_model.train_classifier(sig, grp, str(tmp_path / 'm.npz'), clf)
    assert called['n'] == 2 * min((y == 0).sum(), (y == 1).sum())
    with pytest.raises(ValueError, match='unknown classifier'):
        train_model.train_classifier(sig, grp, str(tmp_path / 'm.npz'), 'XGB')
