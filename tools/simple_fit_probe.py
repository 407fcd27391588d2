"""The LR and NBC fits behind `--train -c LR` / `-c NBC`, timed: a sub-model's whole fit (train_model.fit_lr_on_gpu: six liblinear
fits in one mc_lr_fit call; fit_nb_on_gpu: six GaussianNB fits in one mc_nb_fit call), host work included, at config 5's shape
(9 244 balanced rows, 7 features, tools/rf_fit_probe.py's matrix) and at 5*10^4 rows; scikit-learn's cross_val_score + fit of
LogisticRegression(solver='liblinear', penalty='l1') and GaussianNB() on the same rows if it is importable.

  python tools/simple_fit_probe.py [--runs N] [--sk-runs M] [--no-sklearn]

GPU times: host clock around the fit, median of N (>= 3) runs after one warm-up, and the Newton iterations of the six LR fits.
Output: one JSON object on stdout."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import numpy as np  # noqa: E402


def inputs(n):
    from rf_fit_probe import matrix
    X, y, groups = matrix(n, n)
    labs = list(np.array(['A', 'm6A'])[y])
    return X, labs, ['g%d' % g for g in groups]


def time_gpu(dev, fit, X, labs, grps, runs):
    os.environ['MCALLER_SEED'] = '7'
    sigs = X.tolist()
    fit(labs, sigs, grps, True, device=dev)                                   # warm-up (code objects, allocations)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        classes, scores, final = fit(labs, sigs, grps, True, device=dev)
        ts.append(time.perf_counter() - t)
    return dict(median_s=float(np.median(ts)), runs_s=ts, cv_accuracy=float(np.nanmean(scores))), final


def lr_iterations(dev, X, labs, grps):
    from mcaller_amd import train_model
    _, y, jobs, seeds = train_model.cv_jobs(labs, grps, True)
    t = time.perf_counter()
    fits = dev.lr_fit(X, y, jobs, [train_model.platt_seed(s) for s in seeds], **train_model.LR_PARAMS)
    return dict(mc_lr_fit_s=time.perf_counter() - t, n_iter=[f['n_iter'] for f in fits], status=[f['status'] for f in fits])


def time_sklearn(make, X, labs, grps, runs):
    from sklearn.model_selection import GroupKFold, cross_val_score
    ts, out = [], {}
    for _ in range(runs):
        t = time.perf_counter()
        scores = cross_val_score(make(), X, labs, cv=GroupKFold(n_splits=5), groups=grps)
        cv_s = time.perf_counter() - t
        est = make().fit(X, labs)
        ts.append(time.perf_counter() - t)
        out = dict(cv_s=cv_s, fit_s=ts[-1] - cv_s, cv_accuracy=float(np.mean(scores)))
        if hasattr(est, 'n_iter_'):
            out['n_iter'] = int(np.asarray(est.n_iter_).max())
    return dict(median_s=float(np.median(ts)), runs_s=ts, **out)


def main():
    args = sys.argv[1:]
    runs = max(3, int(args[args.index('--runs') + 1])) if '--runs' in args else 5
    sk_runs = int(args[args.index('--sk-runs') + 1]) if '--sk-runs' in args else 3
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
    for name, n in (('config5', 9244), ('rows_5e4', 50000)):
        X, labs, grps = inputs(n)
        r = dict(rows=n)
        r['lr_gpu'], _ = time_gpu(dev, train_model.fit_lr_on_gpu, X, labs, grps, runs)
        r['lr_gpu'].update(lr_iterations(dev, X, labs, grps))
        r['nb_gpu'], _ = time_gpu(dev, train_model.fit_nb_on_gpu, X, labs, grps, runs)
        if have_sk:
            from sklearn.linear_model import LogisticRegression
            from sklearn.naive_bayes import GaussianNB
            r['lr_sklearn'] = time_sklearn(lambda: LogisticRegression(solver='liblinear', penalty='l1'), X, labs, grps, sk_runs)
            r['nb_sklearn'] = time_sklearn(GaussianNB, X, labs, grps, sk_runs)
        result['shapes'][name] = r
        print(json.dumps({name: r}), file=sys.stderr, flush=True)
    dev.close()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
