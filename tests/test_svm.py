"""`-c SVM` model files (train_model.py:51-53: SVC(kernel='rbf', probability=True)) read without scikit-learn, and the numpy
restatement of libsvm's predict_proba (tests/svm_oracle.py) against scikit-learn's own answers captured by
tests/golden/make_golden_svm.py (tests/golden/svm/)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import svm_oracle

SVM = os.path.join(H.GOLDEN, 'svm')


def meta():
    return json.load(open(os.path.join(SVM, 'svm_meta.json')))


def load(name):
    from mcaller_amd.model_io import load_model_file
    return load_model_file(os.path.join(SVM, name))


def test_model_files_load_without_sklearn(monkeypatch):
    for name in list(sys.modules):
        if name == 'sklearn' or name.startswith('sklearn.'):
            monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, 'sklearn', None)        # any import of it fails
    ms = load('svm_twobase_model_SVM_6_m6A.pkl')
    assert ms.twobase and ms.keys() == ['MG', 'MH']
    n_sv = meta()['n_sv']
    for key, w in ms.models.items():
        assert w.kind == 'svm' and w.n_in == 7 and w.n_sv == n_sv[key] and w.classes == ['A', 'm6A']
        assert w.sv.shape == (w.n_sv, 7) and w.dual_coef.shape == (w.n_sv,) and w.gamma > 0.0
    assert ms.models['MG'].n_sv != ms.models['MH'].n_sv
    g = load('svm_model_SVM_6_m6A.pkl')
    assert not g.twobase and g.keys() == ['general'] and g.models['general'].kind == 'svm'


@pytest.mark.parametrize('name,key', [('svm_twobase_model_SVM_6_m6A.pkl', 'MG'), ('svm_twobase_model_SVM_6_m6A.pkl', 'MH'),
                                      ('svm_model_SVM_6_m6A.pkl', 'general')])
def test_numpy_restatement_matches_known_answers(name, key):
    m = meta()
    w = load(name).models[key]
    X = np.array(m['probes'][key])
    want = np.array(m['known_answers'][key])
    p = svm_oracle.proba(w, X)
    assert np.abs(p - want).max() <= 1e-12, np.abs(p - want).max()
    assert (p > 0.5).any() and (p < 0.5).any() and 0.0 < p.min() and p.max() < 1.0
    # the two-class coupling is libsvm's iteration, not p = 1 - s: the closed form is off by more than the tolerance somewhere
    s = svm_oracle.pairwise(svm_oracle.decision(w.sv, w.dual_coef, w.gamma, w.intercept, X), w.A, w.B)
    assert np.abs((1.0 - s) - want).max() > 1e-4


@pytest.mark.parametrize('key', ['MG', 'MH', 'general'])
def test_in_band_probes_are_exactly_one_half(key):
    m = meta()
    name = 'svm_model_SVM_6_m6A.pkl' if key == 'general' else 'svm_twobase_model_SVM_6_m6A.pkl'
    w = load(name).models[key]
    X = np.array(m['probes'][key])
    p = svm_oracle.proba(w, X)
    inside, near = m['in_band'][key], m['near_band'][key]
    assert len(inside) >= 3 and len(near) >= 2
    assert all(m['known_answers'][key][i] == 0.5 for i in inside)
    assert all(p[i] == 0.5 for i in inside)
    assert all(p[i] != 0.5 and abs(p[i] - m['known_answers'][key][i]) <= 1e-12 for i in near)


@pytest.mark.parametrize('tag,what', [('linear', 'kernel'), ('noprob', 'probability'), ('3class', 'classes')])
def test_unsupported_svcs_are_refused(tag, what):
    with pytest.raises(NotImplementedError, match=what):
        load('unsupported_%s.pkl' % tag)


def test_generator_reproduces_the_committed_fixtures(tmp_path):
    sklearn = pytest.importorskip('sklearn')
    if sklearn.__version__ != meta()['sklearn']:
        pytest.skip('fixtures were made with scikit-learn %s, this is %s' % (meta()['sklearn'], sklearn.__version__))
    r = subprocess.run([sys.executable, os.path.join(H.GOLDEN, 'make_golden_svm.py'), '--out', str(tmp_path)],
                       capture_output=True, text=True, timeout=900, cwd=H.REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    made = tmp_path / 'tests' / 'golden' / 'svm'
    names = sorted(os.listdir(made))
    assert names == sorted(os.listdir(SVM))
    for name in names:
        assert (made / name).read_bytes() == open(os.path.join(SVM, name), 'rb').read(), name
