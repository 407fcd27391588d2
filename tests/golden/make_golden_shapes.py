#!/usr/bin/env python3
"""Generate the five-input model files (tests/golden/shapes/): `-n 4` models of every classifier the HIP path scores besides the
MLP -- RandomForestClassifier with the reference's hyper-parameters (train_model.py:40-45, as make_golden.py's RF fixture),
LogisticRegression(liblinear, l1), GaussianNB and SVC(rbf, probability=True) -- each a dict {'MG': ..., 'MH': ...} (the reference's
two-base format), and a forest of four trees whose probabilities are multiples of small fractions (exact ties of np.round(p, 2)
and of the label p >= 0.5).  Needs scikit-learn, not the reference.

The training rows are seeded synthetic vectors (four slot means and a read quality) labelled by a fixed linear rule with noise;
a few hundred per sub-model keep the files small.

usage: make_golden_shapes.py [--out DIR]   (--out DIR: write under DIR/tests/golden/shapes instead of into the repository)

Outputs (all data):
  shapes_twobase_model_{RF,RF4,LR,NBC,SVM}_4_m6A.pkl
  shapes_meta.json   the scikit-learn version, the number of inputs, trees per forest
"""
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
N_IN = 5
N_FIT = {'MG': 160, 'MH': 240}


def training_rows(rng, n, key):
    import numpy as np
    X = np.round(np.concatenate([rng.normal(0, 2.5, size=(n, N_IN - 1)), rng.uniform(7, 12, size=(n, 1))], axis=1), 4)
    w = np.array([0.9, -0.6, 0.4, 0.3, -0.2]) if key == 'MG' else np.array([-0.5, 0.8, 0.2, -0.7, 0.15])
    y = np.where(X @ w + 1.9 * (key == 'MG') - 1.3 * (key == 'MH') + rng.normal(0, 1.0, size=n) >= 0.0, 'm6A', 'A')
    return X, y


def main():
    import numpy as np
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.linear_model import LogisticRegression
    from sklearn.naive_bayes import GaussianNB
    from sklearn.svm import SVC
    out = os.path.join(os.path.abspath(sys.argv[sys.argv.index('--out') + 1]), 'tests', 'golden') if '--out' in sys.argv else HERE
    outdir = os.path.join(out, 'shapes')
    os.makedirs(outdir, exist_ok=True)
    makers = {
        'RF': lambda: RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=10, max_features=4, min_samples_leaf=2,
                                             min_samples_split=3, n_estimators=20, random_state=3),
        # (grown to the end, two features per split: leaves of two rows, 1/2 among them, in four trees -- means of eighths)
        'RF4': lambda: RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=None, max_features=2, min_samples_leaf=2,
                                              min_samples_split=3, n_estimators=4, random_state=3),
        'LR': lambda: LogisticRegression(solver='liblinear', penalty='l1', random_state=5),
        'NBC': lambda: GaussianNB(),
        'SVM': lambda: SVC(kernel='rbf', probability=True, random_state=7),
    }
    meta = {'sklearn': sklearn.__version__, 'n_in': N_IN, 'n_trees': {}}
    for tag, make in makers.items():
        rng = np.random.default_rng(31)
        models = {}
        for key in ('MG', 'MH'):
            X, y = training_rows(rng, N_FIT[key], key)
            est = make().fit(X, y)
            assert list(est.classes_) == ['A', 'm6A']
            models[key] = est
        if tag.startswith('RF'):
            meta['n_trees'][tag] = len(models['MG'].estimators_)
        with open(os.path.join(outdir, 'shapes_twobase_model_%s_4_m6A.pkl' % tag), 'wb') as fh:
            pickle.dump(models, fh, protocol=4)
    with open(os.path.join(outdir, 'shapes_meta.json'), 'w') as fh:
        json.dump(meta, fh, sort_keys=True)


if __name__ == '__main__':
    main()
