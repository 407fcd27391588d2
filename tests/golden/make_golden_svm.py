#!/usr/bin/env python3
"""Generate the `-c SVM` fixtures (tests/golden/svm/): scikit-learn SVC(kernel='rbf', probability=True) model files -- the
reference's `-c SVM` fit (train_model.py:51-53) -- and scikit-learn's own predict_proba on probe vectors.  Needs scikit-learn,
not the reference.

The training vectors are seeded synthetic rows (six slot means and a read quality) labelled by the committed r95 MLP
(tests/golden/models/r95_twobase_model_NN_6_m6A.pkl, read with mcaller_amd.model_io), as make_golden.py's RF / LR / NBC
fixtures are.  MG and MH are fitted on different numbers of rows, so they have different numbers of support vectors.

usage: make_golden_svm.py [--out DIR]   (--out DIR: write under DIR/tests/golden/svm instead of into the repository)

Outputs (all data):
  svm_twobase_model_SVM_6_m6A.pkl  dict {'MG': SVC, 'MH': SVC} (the reference's two-base format)
  svm_model_SVM_6_m6A.pkl          a bare SVC (read as the 'general' model)
  unsupported_{linear,noprob,3class}.pkl   SVCs the HIP path refuses: kernel='linear', probability=False, three classes
  svm_meta.json                    probes, predict_proba[:, 1] per model, which probes sit in / just outside the band
                                   (0.495, 0.505) of the pairwise probability, the scikit-learn version
"""
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

N_FIT = {'MG': 300, 'MH': 700, 'general': 500}


def mlp_labeller():
    """p(m6A) of the committed r95 model, numpy forward (tanh hidden layer, logistic output)."""
    import numpy as np
    from mcaller_amd.model_io import load_model_file
    ms = load_model_file(os.path.join(HERE, 'models', 'r95_twobase_model_NN_6_m6A.pkl'))

    def p(key, X):
        w = ms.models[key]
        h = np.tanh(X @ w.W1 + w.b1)
        return 1.0 / (1.0 + np.exp(-(h @ w.W2 + w.b2[0])))
    return p


def training_rows(rng, n, label, key):
    import numpy as np
    X = np.round(np.concatenate([rng.normal(0, 2.5, size=(n, 6)), rng.uniform(6, 12, size=(n, 1))], axis=1), 4)
    y = np.where(label(key, X) + rng.normal(0, 0.15, size=n) >= 0.5, 'm6A', 'A')
    return X, y


def band_probes(est, rng, targets):
    """Rows whose pairwise probability s (libsvm's sigmoid of the decision value, before the coupling) is the target: bisection
    on the segment between a row with s below and one with s above."""
    import numpy as np
    from mcaller_amd.model_io import _svc_weights
    from tests import svm_oracle
    w = _svc_weights(est, 'fixture')
    s_of = lambda X: svm_oracle.pairwise(svm_oracle.decision(w.sv, w.dual_coef, w.gamma, w.intercept, X), w.A, w.B)
    cand = np.concatenate([rng.normal(0, 2.5, size=(64, 6)), rng.uniform(6, 12, size=(64, 1))], axis=1)
    s = s_of(cand)
    lo, hi = cand[int(np.argmin(s))], cand[int(np.argmax(s))]
    out = []
    for t in targets:
        a, b = lo.copy(), hi.copy()
        for _ in range(200):
            m = 0.5 * (a + b)
            if s_of(m[None])[0] < t:
                a = m
            else:
                b = m
        out.append(0.5 * (a + b))
    return np.array(out)


def main():
    import numpy as np
    import sklearn
    from sklearn.svm import SVC
    out = os.path.join(os.path.abspath(sys.argv[sys.argv.index('--out') + 1]), 'tests', 'golden') if '--out' in sys.argv else HERE
    outdir = os.path.join(out, 'svm')
    os.makedirs(outdir, exist_ok=True)
    label = mlp_labeller()
    rng = np.random.default_rng(21)
    probes = np.round(np.concatenate([rng.normal(0, 2.5, size=(256, 6)), rng.uniform(6, 12, size=(256, 1))], axis=1), 4)
    probes[0, :6] = 40.0                                   # (far out: every kernel value underflows to 0, dec = intercept)
    probes[1, :6] = -40.0
    probes[2] = 1e3
    inside, outside = [0.4955, 0.4985, 0.5, 0.5015, 0.5045], [0.4945, 0.49, 0.5055, 0.51]
    meta = {'sklearn': sklearn.__version__, 'known_answers': {}, 'n_sv': {}, 'in_band': {}, 'near_band': {}}
    models = {}
    for key in ('MG', 'MH', 'general'):
        X, y = training_rows(rng, N_FIT[key], label, 'MG' if key == 'MG' else 'MH')
        est = SVC(kernel='rbf', probability=True, random_state=7)
        est.fit(X, y)
        assert list(est.classes_) == ['A', 'm6A']
        models[key] = est
        meta['n_sv'][key] = int(est.support_vectors_.shape[0])
    # per model: the shared probes, then its own rows in and just outside the band
    meta['probes'] = {}
    for key, est in models.items():
        band = band_probes(est, rng, inside + outside)
        P = np.concatenate([probes, band])
        meta['probes'][key] = [[float(v) for v in r] for r in P]
        meta['known_answers'][key] = [float(v) for v in est.predict_proba(P)[:, 1]]
        meta['in_band'][key] = list(range(len(probes), len(probes) + len(inside)))
        meta['near_band'][key] = list(range(len(probes) + len(inside), len(P)))
    with open(os.path.join(outdir, 'svm_twobase_model_SVM_6_m6A.pkl'), 'wb') as fh:
        pickle.dump({'MG': models['MG'], 'MH': models['MH']}, fh, protocol=4)
    with open(os.path.join(outdir, 'svm_model_SVM_6_m6A.pkl'), 'wb') as fh:
        pickle.dump(models['general'], fh, protocol=4)
    # what the HIP path refuses (small fits)
    X, y = training_rows(rng, 120, label, 'MH')
    bad = {'linear': SVC(kernel='linear', probability=True, random_state=7).fit(X, y),
           'noprob': SVC(kernel='rbf', probability=False, random_state=7).fit(X, y),
           '3class': SVC(kernel='rbf', probability=True, random_state=7).fit(X, np.where(X[:, 6] > 10, 'x', y))}
    for tag, est in bad.items():
        with open(os.path.join(outdir, 'unsupported_%s.pkl' % tag), 'wb') as fh:
            pickle.dump({'MG': est, 'MH': est}, fh, protocol=4)
    with open(os.path.join(outdir, 'svm_meta.json'), 'w') as fh:
        json.dump(meta, fh)


if __name__ == '__main__':
    main()
