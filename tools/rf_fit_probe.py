"""The random-forest fit behind `--train -c RF`, timed: the six fits of a sub-model (5 GroupKFold folds + the final fit, 50 trees
each, the reference's settings, train_model.py:39-45) in one mc_forest_fit call, at config 5's shape (9 244 balanced rows, 7 features)
and at 5*10^4 rows, on seeded synthetic matrices; scikit-learn's RandomForestClassifier on the same fits if it is importable.

  python tools/rf_fit_probe.py [--runs N] [--sk-runs M] [--no-sklearn] [--file-to-file ROWS]

GPU times: host clock around the synchronous call, median of N (>= 5) runs after one warm-up.  --file-to-file ROWS: also
`mCaller -p positions --train -c RF` on a ROWS-event synthetic file (tools/config5.py's inputs), file to file.  Output: one JSON
object on stdout."""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

RF = dict(n_trees=50, max_depth=10, max_features=4, min_samples_split=3, min_samples_leaf=2, bootstrap=True)


def matrix(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 7)) * np.array([1.5, 2.0, 1.0, 3.0, 1.5, 0.5, 0.0]) + np.array([0, 0, 0, 0, 0, 1.0, 0])
    X[:, 6] = np.round(7.0 + rng.normal(size=n), 6)             # (per-read quality: repeats across a read's rows)
    z = 0.8 * X[:, 0] - 0.4 * X[:, 1] + np.sin(X[:, 2]) + 0.2 * X[:, 3] * X[:, 4]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.uint8)
    groups = rng.integers(0, max(10, n // 40), n)
    return X, y, groups


def jobs_of(y, groups):
    from mcaller_amd.train_model import group_kfold
    fold = group_kfold(groups, 5)
    rows = np.arange(len(y))
    return [(rows[fold != f], rows[fold == f]) for f in range(5)] + [(rows, rows[:0])]


def time_gpu(dev, X, y, jobs, runs):
    seeds = [(7 + 0x9E3779B97F4A7C15 * j) % (1 << 64) for j in range(6)]
    dev.forest_fit(X, y, jobs, seeds=seeds, **RF)                 # warm-up (code objects, allocations)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fits = dev.forest_fit(X, y, jobs, seeds=seeds, **RF)
        ts.append(time.perf_counter() - t)
    nodes = [int(f['tree_off'][-1]) for f in fits]
    acc = [f['val_correct'] / float(f['n_val']) for f in fits[:5]]
    return dict(median_s=float(np.median(ts)), runs_s=ts, nodes_per_tree=float(np.mean(nodes)) / RF['n_trees'], cv_accuracy=float(np.mean(acc)))


def time_sklearn(X, y, jobs, runs):
    from sklearn.ensemble import RandomForestClassifier
    ts, acc = [], []
    for _ in range(runs):
        t = time.perf_counter()
        for tr, va in jobs:
            rf = RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=10, max_features=4, min_samples_leaf=2,
                                        min_samples_split=3, n_estimators=50).fit(X[tr], y[tr])
            if len(va):
                acc.append(float((rf.predict(X[va]) == y[va]).mean()))
        ts.append(time.perf_counter() - t)
    return dict(median_s=float(np.median(ts)), runs_s=ts, cv_accuracy=float(np.mean(acc)))


def file_to_file(rows, runs):
    """`mCaller -p positions --train -c RF` on tools/config5.py's synthetic inputs."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import config5
    from mcaller_amd import mCaller, train_model
    os.environ.setdefault('MCALLER_SEED', '7')
    d = tempfile.mkdtemp(prefix='mc_rf_f2f_')
    paths, _ = config5.write_inputs(rows, d)
    clock = {}
    real = train_model.train_classifier

    def timed(*a, **kw):
        t = time.perf_counter()
        try:
            return real(*a, **kw)
        finally:
            clock['train_classifier_s'] = time.perf_counter() - t

    train_model.train_classifier = timed
    out = []
    try:
        for _ in range(runs):
            model = os.path.join(d, 'trained_model_RF_6_m6A.pkl')
            buf = io.StringIO()
            t = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                mCaller.main(['-p', paths['positions'], '-r', paths['fasta'], '-e', paths['tsv'], '-f', paths['fastq'], '--train',
                              '-c', 'RF', '-d', model])
            dt = time.perf_counter() - t
            line = [ln for ln in buf.getvalue().splitlines() if ln.startswith('Cross validation accuracy')]
            out.append(dict(seconds=dt, train_classifier_s=clock.get('train_classifier_s'), cv_line=line[-1] if line else None))
    finally:
        train_model.train_classifier = real
    return dict(rows=rows, runs=out, median_s=float(np.median([r['seconds'] for r in out[1:] or out])))


def main():
    args = sys.argv[1:]
    runs = max(5, int(args[args.index('--runs') + 1])) if '--runs' in args else 7
    sk_runs = int(args[args.index('--sk-runs') + 1]) if '--sk-runs' in args else 1
    f2f = int(float(args[args.index('--file-to-file') + 1])) if '--file-to-file' in args else 0
    from mcaller_amd.device import Device
    dev = Device(0)
    have_sk = False
    if '--no-sklearn' not in args:
        try:
            import sklearn  # noqa: F401
            have_sk = True
        except ImportError:
            pass
    result = dict(params=RF, shapes={})
    for name, n in (('config5', 9244), ('rows_5e4', 50000)):
        X, y, groups = matrix(n, n)
        jobs = jobs_of(y, groups)
        r = dict(rows=n, gpu=time_gpu(dev, X, y, jobs, runs))
        if have_sk:
            r['sklearn'] = time_sklearn(X, y, jobs, sk_runs)
            r['speedup'] = r['sklearn']['median_s'] / r['gpu']['median_s']
        result['shapes'][name] = r
        print(json.dumps({name: r}), file=sys.stderr)
    if f2f:
        result['train_rf_file_to_file'] = file_to_file(f2f, 2)
    dev.close()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
