"""The fits behind `--train -c RF | SVM | LR | NBC`, timed: a sub-model's whole fit (train_model.fit_*_on_gpu: the five GroupKFold
fits and the final one -- for SVM its five Platt solves and mc_svm_sigmoid_train too -- in one mc_*_fit call), host work included,
at config 5's shape (9 244 balanced rows, 7 features) and at 5*10^4 rows, on seeded synthetic matrices; scikit-learn's
cross_val_score + fit of the reference's estimator (train_model.py:39-60) on the same rows if it is importable.

  python tools/fit_probe.py -c RF|SVM|LR|NBC [--runs N] [--sk-runs M] [--no-sklearn] [--sk-max-rows R] [--file-to-file ROWS]

GPU times: host clock around fit_*_on_gpu with MCALLER_SEED=7, median of N (>= 3) runs after one warm-up; then what one more call
of the Device method tells about the fits (RF: nodes per tree; SVM, LR: iterations and status per solve, the call's own time).
scikit-learn runs only up to R rows (default: no limit; SVM 10^4, its cost grows about as n^2).  --file-to-file ROWS (RF): also
`mCaller -p positions --train -c RF` on a ROWS-event synthetic file (tools/config5.py's inputs), file to file.  Output: one JSON
object on stdout, a line per shape on stderr."""
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


def matrix(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 7)) * np.array([1.5, 2.0, 1.0, 3.0, 1.5, 0.5, 0.0]) + np.array([0, 0, 0, 0, 0, 1.0, 0])
    X[:, 6] = np.round(7.0 + rng.normal(size=n), 6)             # (per-read quality: repeats across a read's rows)
    z = 0.8 * X[:, 0] - 0.4 * X[:, 1] + np.sin(X[:, 2]) + 0.2 * X[:, 3] * X[:, 4]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.uint8)
    groups = rng.integers(0, max(10, n // 40), n)
    return X, y, groups


def inputs(n):
    X, y, groups = matrix(n, n)
    labs = list(np.array(['A', 'm6A'])[y])
    return X, labs, ['g%d' % g for g in groups]


def rf_extras(dev, X, y, jobs, seeds, tm):
    fits = dev.forest_fit(X, y, jobs, seeds=seeds, **tm.RF_PARAMS)
    return dict(nodes_per_tree=float(np.mean([int(f['tree_off'][-1]) for f in fits])) / tm.RF_PARAMS['n_trees'])


def svm_extras(dev, X, y, jobs, seeds, tm):
    plan = tm.svm_plan(X, y, jobs, seeds[5])
    t = time.perf_counter()
    fits = dev.svm_fit(X, y, plan['device'], plan['gammas'], **tm.SVM_PARAMS)
    return dict(mc_svm_fit_s=time.perf_counter() - t, n_iter=[f['n_iter'] for f in fits], status=[f['status'] for f in fits])


def lr_extras(dev, X, y, jobs, seeds, tm):
    t = time.perf_counter()
    fits = dev.lr_fit(X, y, jobs, [tm.platt_seed(s) for s in seeds], **tm.LR_PARAMS)
    return dict(mc_lr_fit_s=time.perf_counter() - t, n_iter=[f['n_iter'] for f in fits], status=[f['status'] for f in fits])


def sk_estimator(clf):
    if clf == 'RF':
        from sklearn.ensemble import RandomForestClassifier
        return RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=10, max_features=4, min_samples_leaf=2,
                                      min_samples_split=3, n_estimators=50)
    if clf == 'SVM':
        from sklearn.svm import SVC
        return SVC(kernel='rbf', probability=True)
    if clf == 'LR':
        from sklearn.linear_model import LogisticRegression
        return LogisticRegression(solver='liblinear', penalty='l1')
    from sklearn.naive_bayes import GaussianNB
    return GaussianNB()


# per classifier: the fit, the keys of its results in a shape's object, one more Device call's figures, what the final fit and
# scikit-learn's estimator add, defaults of --runs / --sk-runs / --sk-max-rows
PROBES = {
    'RF': dict(fit='fit_rf_on_gpu', gpu='gpu', sklearn='sklearn', extras=rf_extras, of_fit=lambda fit: {}, of_est=lambda est: {},
               runs=7, sk_runs=1, sk_max=1 << 62),
    'SVM': dict(fit='fit_svm_on_gpu', gpu='gpu', sklearn='sklearn', extras=svm_extras,
                of_fit=lambda fit: dict(n_sv_final=int(len(fit['support']))),
                of_est=lambda est: dict(n_iter=int(est.n_iter_[0]), n_sv_final=int(len(est.support_))), runs=5, sk_runs=1, sk_max=10000),
    'LR': dict(fit='fit_lr_on_gpu', gpu='lr_gpu', sklearn='lr_sklearn', extras=lr_extras, of_fit=lambda fit: {},
               of_est=lambda est: dict(n_iter=int(np.asarray(est.n_iter_).max())), runs=5, sk_runs=3, sk_max=1 << 62),
    'NBC': dict(fit='fit_nb_on_gpu', gpu='nb_gpu', sklearn='nb_sklearn', extras=None, of_fit=lambda fit: {}, of_est=lambda est: {},
                runs=5, sk_runs=3, sk_max=1 << 62),
}


def time_gpu(dev, probe, X, labs, grps, runs):
    from mcaller_amd import train_model as tm
    os.environ['MCALLER_SEED'] = '7'
    fit_on_gpu = getattr(tm, probe['fit'])
    sigs = X.tolist()
    fit_on_gpu(labs, sigs, grps, True, device=dev)                            # warm-up (code objects, allocations)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        classes, scores, fit = fit_on_gpu(labs, sigs, grps, True, device=dev)
        ts.append(time.perf_counter() - t)
    out = dict(median_s=float(np.median(ts)), runs_s=ts, cv_accuracy=float(np.nanmean(scores)), **probe['of_fit'](fit))
    if probe['extras']:
        _, y, jobs, seeds = tm.cv_jobs(labs, grps, True)
        out.update(probe['extras'](dev, X, y, jobs, seeds, tm))
    return out


def time_sklearn(clf, probe, X, labs, grps, runs):
    from sklearn.model_selection import GroupKFold, cross_val_score
    ts, out = [], {}
    for _ in range(runs):
        t = time.perf_counter()
        scores = cross_val_score(sk_estimator(clf), X, labs, cv=GroupKFold(n_splits=5), groups=grps)
        cv_s = time.perf_counter() - t
        est = sk_estimator(clf).fit(X, labs)
        ts.append(time.perf_counter() - t)
        out = dict(cv_s=cv_s, fit_s=ts[-1] - cv_s, cv_accuracy=float(np.mean(scores)), **probe['of_est'](est))
    return dict(median_s=float(np.median(ts)), runs_s=ts, **out)


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
    clf = args[args.index('-c') + 1] if '-c' in args else None
    if clf not in PROBES:
        sys.exit('usage: fit_probe.py -c RF|SVM|LR|NBC [--runs N] [--sk-runs M] [--no-sklearn] [--sk-max-rows R] [--file-to-file ROWS]')
    probe = PROBES[clf]
    number = lambda flag, default: int(float(args[args.index(flag) + 1])) if flag in args else default        # noqa: E731
    runs, sk_runs, sk_max = max(3, number('--runs', probe['runs'])), number('--sk-runs', probe['sk_runs']), number('--sk-max-rows', probe['sk_max'])
    f2f = number('--file-to-file', 0) if clf == 'RF' else 0
    from mcaller_amd import train_model
    from mcaller_amd.device import Device
    dev = Device(0)
    have_sk = False
    if '--no-sklearn' not in args:
        try:
            import sklearn  # noqa: F401
            have_sk = True
        except ImportError:
            pass
    result = dict(shapes={})
    if clf == 'RF':
        result['params'] = train_model.RF_PARAMS
    for name, n in (('config5', 9244), ('rows_5e4', 50000)):
        X, labs, grps = inputs(n)
        r = {'rows': n, probe['gpu']: time_gpu(dev, probe, X, labs, grps, runs)}
        if have_sk and n <= sk_max:
            r[probe['sklearn']] = time_sklearn(clf, probe, X, labs, grps, sk_runs)
            if clf in ('RF', 'SVM'):
                r['speedup'] = r[probe['sklearn']]['median_s'] / r[probe['gpu']]['median_s']
        result['shapes'][name] = r
        print(json.dumps({name: r}), file=sys.stderr, flush=True)
    if f2f:
        result['train_rf_file_to_file'] = file_to_file(f2f, 2)
    dev.close()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
