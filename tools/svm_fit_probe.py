"""The RBF SVC fit behind `--train -c SVM`, timed: a sub-model's whole fit (train_model.fit_svm_on_gpu: the five GroupKFold solves,
the final solve and its five Platt solves in one mc_svm_fit call, then mc_svm_sigmoid_train), host work included, at config 5's
shape (9 244 balanced rows, 7 features, tools/rf_fit_probe.py's matrix) and at 5*10^4 rows; scikit-learn's cross_val_score +
fit of SVC(kernel='rbf', probability=True) on the same rows if it is importable.

  python tools/svm_fit_probe.py [--runs N] [--sk-runs M] [--no-sklearn] [--sk-max-rows R]

GPU times: host clock around fit_svm_on_gpu, median of N (>= 3) runs after one warm-up; the solves' iteration counts and support
vectors of the final fit.  scikit-learn runs only up to R rows (default 10^4; its cost grows about as n^2).  Output: one JSON object
on stdout."""
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


def time_gpu(dev, X, labs, grps, runs):
    from mcaller_amd import train_model
    os.environ['MCALLER_SEED'] = '7'
    sigs = X.tolist()
    train_model.fit_svm_on_gpu(labs, sigs, grps, True, device=dev)          # warm-up (code objects, allocations)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        classes, scores, fit = train_model.fit_svm_on_gpu(labs, sigs, grps, True, device=dev)
        ts.append(time.perf_counter() - t)
    _, y, jobs, seeds = train_model.cv_jobs(labs, grps, True)
    plan = train_model.svm_plan(X, y, jobs, seeds[5])
    t = time.perf_counter()
    fits = dev.svm_fit(X, y, plan['device'], plan['gammas'], **train_model.SVM_PARAMS)
    solve_s = time.perf_counter() - t
    return dict(median_s=float(np.median(ts)), runs_s=ts, mc_svm_fit_s=solve_s, n_iter=[f['n_iter'] for f in fits],
                status=[f['status'] for f in fits], n_sv_final=int(len(fit['support'])), cv_accuracy=float(np.nanmean(scores)))


def time_sklearn(X, labs, grps, runs):
    from sklearn.model_selection import GroupKFold, cross_val_score
    from sklearn.svm import SVC
    ts, out = [], {}
    for _ in range(runs):
        t = time.perf_counter()
        scores = cross_val_score(SVC(kernel='rbf', probability=True), X, labs, cv=GroupKFold(n_splits=5), groups=grps)
        cv_s = time.perf_counter() - t
        est = SVC(kernel='rbf', probability=True).fit(X, labs)
        ts.append(time.perf_counter() - t)
        out = dict(cv_s=cv_s, fit_s=ts[-1] - cv_s, n_iter=int(est.n_iter_[0]), n_sv_final=int(len(est.support_)),
                   cv_accuracy=float(np.mean(scores)))
    return dict(median_s=float(np.median(ts)), runs_s=ts, **out)


def main():
    args = sys.argv[1:]
    runs = max(3, int(args[args.index('--runs') + 1])) if '--runs' in args else 5
    sk_runs = int(args[args.index('--sk-runs') + 1]) if '--sk-runs' in args else 1
    sk_max = int(float(args[args.index('--sk-max-rows') + 1])) if '--sk-max-rows' in args else 10000
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
        r = dict(rows=n, gpu=time_gpu(dev, X, labs, grps, runs))
        if have_sk and n <= sk_max:
            r['sklearn'] = time_sklearn(X, labs, grps, sk_runs)
            r['speedup'] = r['sklearn']['median_s'] / r['gpu']['median_s']
        result['shapes'][name] = r
        print(json.dumps({name: r}), file=sys.stderr, flush=True)
    dev.close()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
