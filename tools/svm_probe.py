"""`-c SVM` (k3_svm) on a synthetic table: full passes (strand resolve, scan, emit, classifier) timed with the fixture SVM
(tests/golden/svm, ~200 / ~330 support vectors), a synthetic 10^4-support-vector SVM and the shipped NN on the same table; per
model ms per pass, support-vector evaluations per second, and scikit-learn's predict_proba on the same feature rows over 16
processes (where scikit-learn is installed; measured before the GPU is touched).

usage: svm_probe.py [rows=2e6] [--passes N] [--only fixture|svm10k|nn] [--no-sklearn] [--json]
       svm_probe.py --share <rocprofv3 kernel_stats.csv>    the k3_svm share of the kernel time of a run under
                                                           `rocprofv3 --kernel-trace --stats` (a run of its own: --only, --no-sklearn)"""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN_SVM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'svm')
N_SV_SYNTH = 10000


def share(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r['TotalDurationNs']) for r in rows)
    svm = sum(float(r['TotalDurationNs']) for r in rows if 'k3_svm' in r['Name'])
    calls = sum(int(r['Calls']) for r in rows if 'k3_svm' in r['Name'])
    print('k3_svm: %d calls, %.3f ms of %.3f ms kernel time (%.1f %%)' % (calls, svm / 1e6, tot / 1e6, 100.0 * svm / max(tot, 1.0)))


def synthetic_svm():
    from mcaller_amd.model_io import SVMWeights
    rng = np.random.default_rng(77)
    sv = np.concatenate([rng.normal(0, 2.5, size=(N_SV_SYNTH, 6)), rng.uniform(6, 12, size=(N_SV_SYNTH, 1))], axis=1)
    return SVMWeights(sv, rng.uniform(-1, 1, size=N_SV_SYNTH), 0.017, -0.2, -0.25, -0.1, ['A', 'm6A'])


def models():
    """tag -> (list of weights in sub-model order, uint8[256] key table, scikit-learn estimators or None)."""
    from mcaller_amd.extract_contexts import submodel_setup
    from mcaller_amd.model_io import load_model_file, shipped_model
    out = {}
    ms = load_model_file(os.path.join(GOLDEN_SVM, 'svm_twobase_model_SVM_6_m6A.pkl'))
    _, w, _, soc = submodel_setup(ms, 'A')
    out['fixture'] = (w, soc)
    s = synthetic_svm()
    out['svm10k'] = ([s, s], soc)                  # (MG and MH the same model: every record walks 10^4 support vectors)
    _, w, _, soc_nn = submodel_setup(load_model_file(shipped_model('r95_twobase_model_NN_6_m6A')), 'A')
    out['nn'] = (w, soc_nn)
    return out


def sklearn_estimators(tag, weights):
    """SVC objects that score as `weights` do: the fixture's own, or a small fit whose model is replaced by the synthetic one."""
    import pickle
    from sklearn.svm import SVC
    if tag == 'fixture':
        d = pickle.load(open(os.path.join(GOLDEN_SVM, 'svm_twobase_model_SVM_6_m6A.pkl'), 'rb'))
        return [d['MG'], d['MH']]
    w = weights[0]
    rng = np.random.default_rng(1)
    X = rng.normal(size=(60, 7))
    e = SVC(kernel='rbf', probability=True, random_state=0).fit(X, np.where(X[:, 0] > 0, 'm6A', 'A'))
    n = w.n_sv
    e.support_vectors_, e.support_ = w.sv, np.arange(n, dtype=np.int32)
    e._n_support = np.array([n // 2, n - n // 2], dtype=np.int32)
    e._dual_coef_, e.dual_coef_ = w.dual_coef[None], -w.dual_coef[None]
    e._intercept_, e.intercept_ = np.array([w.intercept]), np.array([-w.intercept])
    e._gamma, e._probA, e._probB = w.gamma, np.array([w.A]), np.array([w.B])
    return [e, e]


def _sk_part(args):
    est, X = args
    return est.predict_proba(X)[:, 1]


def time_sklearn(ests, X, sub, procs=16):
    from concurrent.futures import ProcessPoolExecutor
    jobs = []
    for m, e in enumerate(ests):
        Xm = X[sub == m]
        jobs += [(e, part) for part in np.array_split(Xm, procs) if len(part)]
    with ProcessPoolExecutor(procs) as ex:
        list(ex.map(_sk_part, jobs[:procs]))                # (warm: the workers start, the estimators travel once)
        t = time.perf_counter()
        list(ex.map(_sk_part, jobs))
        return time.perf_counter() - t


def main():
    if '--share' in sys.argv:
        share(sys.argv[sys.argv.index('--share') + 1])
        return
    from mcaller_amd import synth, _lib
    from tests import helpers as H
    n_rows = int(float(sys.argv[1])) if len(sys.argv) > 1 and not sys.argv[1].startswith('-') else 2000000
    passes = int(sys.argv[sys.argv.index('--passes') + 1]) if '--passes' in sys.argv else 20
    only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
    codes = synth.genome()
    ref = synth.SynthRef(codes)
    table, qual = synth.make_table(n_rows, seed=1000, codes=codes)
    M = models()
    tags = [only] if only else ['fixture', 'svm10k', 'nn']
    # the records and their feature rows (the CPU oracle's: the same records the device makes)
    orc = H.oracle_records(table, ref.device_arrays(), qual, 6, 0, 0.0)
    n = orc.n
    info = orc.info[:n]
    scored = (info & (_lib.I_TOO_MANY | _lib.I_EDGE)) == 0
    X = np.zeros((n, 7))
    X[:, :6] = orc.feats[:n * 6].reshape(n, 6)
    X[:, 6] = np.asarray(qual)[table.seg_read[orc.site_seg[:n]]]
    res = {}
    for tag in tags:
        w, soc = M[tag]
        sub = soc[(info >> _lib.I_NEXT_SHIFT) & 0xFF].astype(np.int64)
        sub[~scored] = 255
        ok = sub < len(w)
        evals = int(sum(w[m].n_sv * int((sub == m).sum()) for m in range(len(w)))) if w[0].kind == 'svm' else 0
        res[tag] = dict(records=int(n), scored=int(ok.sum()), sv_evals_per_pass=evals)
        if w[0].kind == 'svm' and '--no-sklearn' not in sys.argv:
            try:
                ests = sklearn_estimators(tag, w)
            except ImportError:
                ests = None
            if ests is not None:
                s = time_sklearn(ests, X[ok], sub[ok])
                res[tag].update(sklearn_16proc_s=s, sklearn_sv_evals_per_s=evals / s)
    from mcaller_amd.device import Device
    dev = Device(0)
    dev.set_reference(ref.device_arrays()); dev.upload_table(table); dev.set_read_quality(qual)
    for tag in tags:
        w, soc = M[tag]
        dev.set_classifier(w, soc)
        for _ in range(3):
            dev.run(6, 0, 0.0)
        dev.sync()
        t = time.perf_counter()
        for _ in range(passes):
            dev.run(6, 0, 0.0)
        dev.sync()
        ms = 1e3 * (time.perf_counter() - t) / passes
        rec = dev.fetch()
        r = res[tag]
        r.update(ms_per_pass=ms, device_records=int(rec.n), classifier_ms=dev.times_ms()['classifier'])
        if r['sv_evals_per_pass']:
            r['sv_evals_per_s'] = r['sv_evals_per_pass'] / (ms / 1e3)
        print('%-8s %8.3f ms/pass  %d records (%d scored)  classifier stage %.3f ms%s%s' % (
            tag, ms, rec.n, r['scored'], r['classifier_ms'],
            ('  %.3g SV evaluations/s' % r['sv_evals_per_s']) if 'sv_evals_per_s' in r else '',
            ('  | scikit-learn, 16 processes: %.3f s, %.3g SV evaluations/s' % (r['sklearn_16proc_s'], r['sklearn_sv_evals_per_s']))
            if 'sklearn_16proc_s' in r else ''))
    dev.close()
    if '--json' in sys.argv:
        print(json.dumps(res))


if __name__ == '__main__':
    main()
