"""`--train`: fit a classifier on the labelled feature matrix the GPU path built (train_model.py:33-113).

`NN` (the default, train_model.py:47) is fitted on the GPU: class balancing (:81-86), 5-fold GroupKFold by context
(:62-65, :92) and the final fit (:100) are six independent runs of the same optimiser, launched together as one
`mc_mlp_fit` call (four workgroups per fit, mcaller_amd/csrc/mc_train.hip).  The optimiser is scikit-learn's
MLPClassifier recipe (Adam, tanh, alpha=0.001, batches of min(200, n), tol/n_iter_no_change stopping); like the
reference's `random_state=None` fit, two runs differ unless MCALLER_SEED is set.

The model file is what the reference writes -- a pickle of {sub-model: MLPClassifier} (:110-112) -- when scikit-learn is
importable (the estimators are filled with the fitted arrays, so the reference can load them); otherwise a neutral
`.npz` of the same arrays that mcaller_amd.model_io reads.

`RF` (train_model.py:39-45, without `min_impurity_split`, which scikit-learn >= 1.0 rejects) is fitted on the GPU too: the same
six jobs, 50 trees each, every tree a workgroup of one `mc_forest_fit` call (mcaller_amd/csrc/mc_forest_fit.hip); its model file
is a pickle of {sub-model: RandomForestClassifier} or the neutral `.npz` of the trees.

`SVM` (train_model.py:51-53: SVC(kernel='rbf', probability=True) with scikit-learn's defaults) is fitted on the GPU as well: the five
fold solves, the final solve and the five solves of its Platt scaling -- eleven SMO solves, a workgroup each of one `mc_svm_fit` call
(mcaller_amd/csrc/mc_svm_fit.hip) -- then libsvm's sigmoid_train on the device.  Its model file is a pickle of {sub-model: SVC} or
the neutral `.npz` of the support vectors.

`LR` (train_model.py:55-57: LogisticRegression(solver='liblinear', penalty='l1')) and `NBC` (:59-60: GaussianNB()) are fitted on the
GPU too: the six jobs of a sub-model, a workgroup each of one `mc_lr_fit` (liblinear's solve_l1r_lr, each fit seeded like scikit-learn's
from its cv_jobs seed) or `mc_nb_fit` call (mcaller_amd/csrc/mc_simple_fit.hip).  Their model files are a pickle of
{sub-model: LogisticRegression | GaussianNB} or the neutral `.npz` of the weights.  No classifier needs scikit-learn to be fitted.
"""
import os
import pickle

import numpy as np


def pos2label(positions):
    """train_model.py:18-20."""
    return {(pos.split()[0], int(pos.split()[1]), pos.split()[2]): pos.split()[3]
            for pos in open(positions, 'r').read().split('\n') if len(pos.split()) > 1}


def group_kfold(groups, n_splits=5):
    """Fold of every sample under scikit-learn's GroupKFold (train_model.py:62-63): groups, largest first, are dealt to
    the currently lightest fold."""
    uniq, inv = np.unique(np.asarray(groups), return_inverse=True)
    if len(uniq) < n_splits:
        raise ValueError('Cannot have number of splits n_splits=%d greater than the number of groups: %d.'
                         % (n_splits, len(uniq)))
    per_group = np.bincount(inv)
    order = np.argsort(per_group)[::-1]
    per_fold = np.zeros(n_splits)
    group_to_fold = np.zeros(len(uniq), dtype=np.int64)
    for gi in order:
        lightest = int(np.argmin(per_fold))
        per_fold[lightest] += per_group[gi]
        group_to_fold[gi] = lightest
    return group_to_fold[inv]


def balanced_rows(signals, groups):
    """train_model.py:81-86: the first min-class-size rows of every label, label by label."""
    num_examples = min([len(signals[label]) for label in signals])
    labs, sigs, grps = [], [], []
    for label in signals:
        labs = labs + [label] * num_examples
        sigs = sigs + signals[label][:num_examples]
        grps = grps + groups[label][:num_examples]
    return labs, sigs, grps


def balanced_arrays(signals, groups):
    """balanced_rows for array leaves (load_mCaller_data.tsv2matrix_device): the same rows as slices of the labels' arrays, put
    together once.  -> (labels: list, float64 [n, features], contexts [n])."""
    num_examples = min([len(signals[label]) for label in signals])
    labs = [label for label in signals for _ in range(num_examples)]
    sigs = np.concatenate([np.asarray(signals[label], dtype=np.float64)[:num_examples] for label in signals])
    grps = np.concatenate([np.asarray(groups[label])[:num_examples] for label in signals])
    return labs, sigs, grps


def _has_array_leaves(signals):
    return len(signals) > 0 and all(isinstance(rows, np.ndarray) for rows in signals.values())


def _shown(rows):
    """The first ten of a balanced column as train_classifier prints them: array rows as lists, 'S' contexts as str."""
    if not isinstance(rows, np.ndarray):
        return rows[:10]
    return [c.decode('ascii') for c in rows[:10].tolist()] if rows.dtype.kind == 'S' else rows[:10].tolist()


def _seed():
    env = os.environ.get('MCALLER_SEED', '')
    return int(env) if env != '' else int.from_bytes(os.urandom(7), 'little')


def cv_jobs(labs, grps, use_groups):
    """The six fits of a sub-model: 5-fold GroupKFold by context (StratifiedKFold without shuffling when there are no groups)
    and the final fit on all rows, with their seeds.  -> (classes, y, jobs, seeds)."""
    classes = sorted(set(labs))                                   # LabelBinarizer order == estimator.classes_
    if len(classes) != 2:
        raise ValueError('training needs exactly two labels in the positions file, got %s' % classes)
    y = np.asarray([1 if lab == classes[1] else 0 for lab in labs], dtype=np.uint8)
    n = len(y)
    if use_groups:
        fold = group_kfold(grps, 5)
    else:                                                         # cv=5 -> StratifiedKFold without shuffling
        fold = np.zeros(n, dtype=np.int64)
        for cls in (0, 1):
            rows = np.nonzero(y == cls)[0]
            fold[rows] = (np.arange(len(rows)) * 5) // max(len(rows), 1)
    rows = np.arange(n)
    jobs = [(rows[fold != f], rows[fold == f]) for f in range(5)] + [(rows, np.zeros(0, dtype=np.int64))]
    seed = _seed()
    return classes, y, jobs, [(seed + 0x9E3779B97F4A7C15 * j) % (1 << 64) for j in range(6)]


def _open_fit(labs, sigs, grps, use_groups, device):
    """What every fit_*_on_gpu starts from -> (device, classes, y, the six cv_jobs, their seeds, X)."""
    from .device import get_device
    dev = device if device is not None else get_device()
    classes, y, jobs, seeds = cv_jobs(labs, grps, use_groups)
    return dev, classes, y, jobs, seeds, np.asarray(sigs, dtype=np.float64)     # (an fp64 array passes through as it is)


def _fold_scores(fits):
    """Cross-validation scores of the folds' fit dicts: held-out accuracy, nan for a fold that was not run (None)."""
    return np.array([np.nan if f is None else f['val_correct'] / float(f['n_val']) for f in fits])


def _two_class_jobs(y, jobs):
    """The jobs, by number, whose training rows hold both classes."""
    return [j for j, (tr, _) in enumerate(jobs) if len(np.unique(y[tr])) == 2]


def fit_nn_on_gpu(labs, sigs, grps, use_groups, device=None, hidden=100):
    """-> (classes, cross-validation scores, final weights dict)."""
    dev, classes, y, jobs, seeds, X = _open_fit(labs, sigs, grps, use_groups, device)
    fits = dev.mlp_fit(X, y, jobs, hidden=hidden, seeds=seeds)
    return classes, _fold_scores(fits[:5]), fits[5]


RF_PARAMS = dict(n_trees=50, max_depth=10, max_features=4, min_samples_split=3, min_samples_leaf=2, bootstrap=True)   # train_model.py:39-45


def fit_rf_on_gpu(labs, sigs, grps, use_groups, device=None):
    """`-c RF`: the six forests of a sub-model in one mc_forest_fit call (k5_forest_fit).  -> (classes, cross-validation scores,
    final forest dict: Device.forest_fit's arrays plus n_features)."""
    dev, classes, y, jobs, seeds, X = _open_fit(labs, sigs, grps, use_groups, device)
    fits = dev.forest_fit(X, y, jobs, seeds=seeds, **RF_PARAMS)
    return classes, _fold_scores(fits[:5]), dict(fits[5], n_features=X.shape[1])


def as_sklearn_estimator(fit, classes, n_samples):
    """A scikit-learn MLPClassifier holding the fitted arrays (what the reference pickles, train_model.py:110-112)."""
    from sklearn.neural_network import MLPClassifier
    from sklearn.preprocessing import LabelBinarizer
    m = MLPClassifier(hidden_layer_sizes=(len(fit['b1'])), alpha=0.001, learning_rate='adaptive', early_stopping=False,
                      activation='tanh')
    m.coefs_ = [np.array(fit['W1'], dtype=np.float64), np.array(fit['W2'], dtype=np.float64).reshape(-1, 1)]
    m.intercepts_ = [np.array(fit['b1'], dtype=np.float64), np.array([fit['b2']], dtype=np.float64)]
    m.n_features_in_ = m.coefs_[0].shape[0]
    m.n_layers_, m.n_outputs_, m.out_activation_ = 3, 1, 'logistic'
    m.classes_ = np.array(classes)
    m._label_binarizer = LabelBinarizer().fit(classes)
    m.loss_curve_ = [float(x) for x in fit['loss_curve']]
    m.loss_ = m.loss_curve_[-1] if m.loss_curve_ else float('nan')
    m.best_loss_ = min(m.loss_curve_) if m.loss_curve_ else float('nan')
    m.n_iter_ = int(fit['n_iter'])
    m.t_ = int(fit['n_iter']) * int(n_samples)
    m.validation_scores_ = None
    m.best_validation_score_ = None
    return m


def as_sklearn_forest(fit, classes):
    """A scikit-learn RandomForestClassifier holding the fitted trees (what the reference pickles for -c RF): every estimator's
    tree_ filled through Tree.__setstate__ with scikit-learn's node records."""
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    from sklearn.tree._tree import NODE_DTYPE, Tree
    p = RF_PARAMS
    d = int(fit['n_features'])
    kw = dict(criterion='entropy', max_depth=p['max_depth'], max_features=p['max_features'], min_samples_leaf=p['min_samples_leaf'],
              min_samples_split=p['min_samples_split'])
    off = fit['tree_off']
    estimators = []
    for t in range(len(off) - 1):
        a, b = int(off[t]), int(off[t + 1])
        nodes = np.zeros(b - a, dtype=NODE_DTYPE)
        nodes['left_child'], nodes['right_child'] = fit['left'][a:b], fit['right'][a:b]
        nodes['feature'], nodes['threshold'] = fit['feature'][a:b], fit['threshold'][a:b]
        nodes['impurity'], nodes['n_node_samples'] = fit['impurity'][a:b], fit['n_node_samples'][a:b]
        nodes['weighted_n_node_samples'] = fit['weighted_n_node_samples'][a:b]
        if 'missing_go_to_left' in NODE_DTYPE.names:
            nodes['missing_go_to_left'] = 0
        tree = Tree(d, np.array([2], dtype=np.intp), 1)
        tree.__setstate__(dict(max_depth=_tree_depth(fit['left'][a:b], fit['right'][a:b]), node_count=b - a, nodes=nodes,
                               values=np.ascontiguousarray(fit['value'][a:b], dtype=np.float64).reshape(b - a, 1, 2)))
        est = DecisionTreeClassifier(**kw)
        est.tree_ = tree
        est.n_features_in_, est.n_outputs_, est.n_classes_ = d, 1, np.intp(2)
        est.classes_ = np.array([0.0, 1.0])
        est.max_features_ = p['max_features']
        estimators.append(est)
    rf = RandomForestClassifier(bootstrap=p['bootstrap'], n_estimators=len(estimators), **kw)
    rf.estimator_ = DecisionTreeClassifier(**kw)
    rf.estimators_ = estimators
    rf.n_features_in_, rf.n_outputs_, rf.n_classes_ = d, 1, 2
    rf.classes_ = np.array(classes)
    return rf


def _tree_depth(left, right):
    depth = np.zeros(len(left), dtype=np.int64)
    for v in range(len(left)):                                    # pre-order: a parent comes before its children
        if left[v] >= 0:
            depth[left[v]] = depth[right[v]] = depth[v] + 1
    return int(depth.max()) if len(depth) else 0


SVM_PARAMS = dict(C=1.0, tol=1e-3)                               # SVC's defaults (train_model.py:51-53)


def svc_gamma(X):
    """gamma='scale' as scikit-learn's SVC.fit resolves it on the rows it is given: 1 / (n_features * X.var()), 1.0 if X.var() is 0."""
    var = X.var()
    return 1.0 / (X.shape[1] * var) if var != 0 else 1.0


def platt_seed(seed):
    """The 31-bit seed of the Platt shuffle: the final job's cv_jobs seed modulo 2^31 - 1 (the range of the seed scikit-learn draws
    for libsvm, RandomState.randint(2**31 - 1))."""
    return int(seed % (2 ** 31 - 1))


class MT19937Draws(object):
    """The generator libsvm and liblinear use in scikit-learn (newrand.h): std::mt19937 seeded once (set_seed), and
    bounded_rand_int(range) by Lemire's method -- a draw whose low word x * range mod 2^32 lies below 2^32 mod range is drawn
    again.  NumPy's MT19937 with its legacy seeding is the same generator.  Draws are taken in order from one stream."""

    def __init__(self, seed):
        self._mt = np.random.MT19937()
        self._mt._legacy_seeding(int(seed))
        self._raw, self._p = np.zeros(0, dtype=np.uint64), 0

    def _have(self, k):
        if len(self._raw) - self._p < k:
            self._raw, self._p = np.concatenate([self._raw[self._p:], self._mt.random_raw(k + 16)]), 0

    def draws(self, ranges):
        """bounded_rand_int(r) for every r of `ranges`, one after another."""
        ranges = np.asarray(ranges, dtype=np.uint64)
        out = np.zeros(len(ranges), dtype=np.int64)
        i = 0
        while i < len(ranges):
            rng = ranges[i:]
            self._have(len(rng))
            m = self._raw[self._p:self._p + len(rng)] * rng
            bad = np.nonzero((m & 0xFFFFFFFF) < (np.uint64(1 << 32) % rng))[0]      # rejected: low word below 2^32 mod range
            ok = len(rng) if len(bad) == 0 else int(bad[0])
            out[i:i + ok] = (m[:ok] >> np.uint64(32)).astype(np.int64)
            i, self._p = i + ok, self._p + ok
            if len(bad):                                                              # redraw this position until accepted
                self._p += 1
                r = ranges[i]
                while True:
                    self._have(1)
                    m1 = self._raw[self._p] * r
                    self._p += 1
                    if (m1 & np.uint64(0xFFFFFFFF)) >= np.uint64(1 << 32) % r:
                        out[i] = int(m1 >> np.uint64(32))
                        i += 1
                        break
        return out

    def draw(self, r):
        return int(self.draws([r])[0])


def libsvm_permutation(l, seed):
    """svm_binary_svc_probability's shuffle: perm[i] <-> perm[i + bounded_rand_int(l - i)] for i = 0 .. l-1 (MT19937Draws)."""
    pick = MT19937Draws(seed).draws(np.arange(l, 0, -1, dtype=np.uint64))
    perm = list(range(l))
    for i in range(l):
        j = i + int(pick[i])
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm, dtype=np.int64)


def svm_plan(X, y, jobs, seed):
    """The solves of a sub-model: the five fold jobs and the final job (their training rows grouped classes_[0]
    first, each fold's own gamma), then the Platt folds of the final fit: its rows grouped classes_[0] first (libsvm's +1), shuffled
    by libsvm_permutation, fold f = positions [f l / 5, (f+1) l / 5); a fold whose complement holds both classes is solved on it
    (classes_[1] first, the sub-problem's sorted labels), one that does not gets dec = +1 / -1 on its held-out rows.
    -> dict(device=[(train, val)], gammas, cv=[device job of fold f, or None when its training rows hold one class], final (its
    device job), order (its rows), perm, platt=[(device job or None, held-out positions, constant dec)], gamma)."""
    group = lambda rows, first: np.concatenate([rows[y[rows] == first], rows[y[rows] != first]])     # noqa: E731
    device, gammas, cv = [], [], []
    run = _two_class_jobs(y, jobs[:5])
    for f, (tr, va) in enumerate(jobs[:5]):
        if f not in run:
            cv.append(None)
            continue
        cv.append(len(device))
        device.append((group(tr, 0), va))
        gammas.append(svc_gamma(X[tr]))
    order = group(np.arange(len(y)), 0)
    gamma = svc_gamma(X)
    final = len(device)
    device.append((order, np.zeros(0, dtype=np.int64)))
    gammas.append(gamma)
    l = len(order)
    perm = libsvm_permutation(l, platt_seed(seed))
    platt = []
    for f in range(5):
        begin, end = f * l // 5, (f + 1) * l // 5
        comp = order[np.concatenate([perm[:begin], perm[end:]])]
        held = perm[begin:end]
        labs = set(y[comp].tolist())
        if len(labs) == 2:
            platt.append((len(device), held, 0.0))
            device.append((group(comp, 1), order[held]))
            gammas.append(gamma)
        else:
            platt.append((None, held, 0.0 if not labs else (1.0 if labs == {0} else -1.0)))
    return dict(device=device, gammas=gammas, cv=cv, final=final, order=order, perm=perm, platt=platt, gamma=gamma)


def fit_svm_on_gpu(labs, sigs, grps, use_groups, device=None):
    """`-c SVM`: a sub-model's eleven SMO solves in one mc_svm_fit call (k6_svm_fit), the Platt parameters by mc_svm_sigmoid_train.
    -> (classes, cross-validation scores, final fit dict: the support vectors and what SVC keeps of them)."""
    dev, classes, y, jobs, seeds, X = _open_fit(labs, sigs, grps, use_groups, device)
    plan = svm_plan(X, y, jobs, seeds[5])
    fits = dev.svm_fit(X, y, plan['device'], plan['gammas'], **SVM_PARAMS)
    scores = _fold_scores([None if j is None else fits[j] for j in plan['cv']])
    order = plan['order']
    dec = np.zeros(len(order))
    for job, held, const in plan['platt']:
        dec[held] = fits[job]['val_dec'] if job is not None else const
    A, B = dev.svm_sigmoid_train(dec, y[order])
    final = fits[plan['final']]
    alpha = final['alpha']
    sv = alpha > 0
    support = order[sv]
    ysolve = np.where(y[order] == 0, 1.0, -1.0)
    fit = dict(support=support.astype(np.int32), sv=X[support], dual_coef=(ysolve * alpha)[sv], intercept=-final['rho'],
               gamma=plan['gamma'], probA=A, probB=B, n_support=np.array([(y[support] == 0).sum(), (y[support] == 1).sum()], np.int32),
               n_iter=final['n_iter'], status=final['status'], n_samples=len(y), n_features=X.shape[1])
    return classes, scores, fit


def as_sklearn_svc(fit, classes):
    """A scikit-learn SVC(kernel='rbf', probability=True) holding the fitted model: every attribute SVC.fit sets, with its dtype and
    shape (the libsvm arrays `_dual_coef_`, `_intercept_` and their public, sign-flipped copies for two classes)."""
    from sklearn.svm import SVC
    m = SVC(kernel='rbf', probability=True)
    m._sparse = False
    m.n_features_in_ = int(fit['n_features'])
    m.classes_ = np.array(classes)
    m.class_weight_ = np.ones(2, dtype=np.float64)
    m.shape_fit_ = (int(fit['n_samples']), int(fit['n_features']))
    m._gamma = np.float64(fit['gamma'])
    m.support_ = np.asarray(fit['support'], dtype=np.int32)
    m.support_vectors_ = np.ascontiguousarray(fit['sv'], dtype=np.float64)
    m._n_support = np.asarray(fit['n_support'], dtype=np.int32)
    m.dual_coef_ = np.asarray(fit['dual_coef'], dtype=np.float64).reshape(1, -1)
    m.intercept_ = np.array([fit['intercept']], dtype=np.float64)
    m._probA = np.array([fit['probA']], dtype=np.float64)
    m._probB = np.array([fit['probB']], dtype=np.float64)
    m.fit_status_ = int(fit['status'])
    m._num_iter = np.array([fit['n_iter']], dtype=np.int32)
    m.n_iter_ = m._num_iter
    m._intercept_ = m.intercept_.copy()
    m._dual_coef_ = m.dual_coef_
    m.intercept_ *= -1                                            # (SVC.fit: two classes flip the public sign)
    m.dual_coef_ = -m.dual_coef_
    return m


LR_PARAMS = dict(C=1.0, tol=1e-4, max_iter=100)                  # LogisticRegression(solver='liblinear', penalty='l1') (train_model.py:55-57)


def fit_lr_on_gpu(labs, sigs, grps, use_groups, device=None):
    """`-c LR`: a sub-model's six liblinear fits in one mc_lr_fit call (k7_lr_fit), each seeded with its cv_jobs seed modulo
    2^31 - 1 (platt_seed's rule, the range of scikit-learn's draw).  A fold whose training rows hold one class scores nan, as
    cross_val_score gives for liblinear's refusal.  -> (classes, cross-validation scores, final fit dict: coef, intercept, n_iter,
    status, n_features)."""
    dev, classes, y, jobs, seeds, X = _open_fit(labs, sigs, grps, use_groups, device)
    run = _two_class_jobs(y, jobs)
    fits = dict(zip(run, dev.lr_fit(X, y, [jobs[j] for j in run], [platt_seed(seeds[j]) for j in run], **LR_PARAMS)))
    final = fits[5]
    fit = dict(coef=final['coef'], intercept=final['intercept'], n_iter=final['n_iter'], status=final['status'], n_features=X.shape[1])
    return classes, _fold_scores([fits.get(f) for f in range(5)]), fit


NB_PARAMS = dict(var_smoothing=1e-9)                              # GaussianNB() (train_model.py:59-60)


def fit_nb_on_gpu(labs, sigs, grps, use_groups, device=None):
    """`-c NBC`: a sub-model's six GaussianNB fits in one mc_nb_fit call (k7_nb_fit).  A fold whose training rows hold one class
    predicts that class everywhere, as the fitted GaussianNB would: its score is the share of held-out rows in it.  -> (classes,
    cross-validation scores, final fit dict: theta, var, epsilon, class_count, class_prior, n_features)."""
    dev, classes, y, jobs, seeds, X = _open_fit(labs, sigs, grps, use_groups, device)
    run = _two_class_jobs(y, jobs)
    fits = dict(zip(run, dev.nb_fit(X, y, [jobs[j] for j in run], **NB_PARAMS)))
    scores = _fold_scores([fits.get(f) for f in range(5)])
    for f, (tr, va) in enumerate(jobs[:5]):
        if f not in fits:
            scores[f] = float(np.mean(y[va] == y[tr[0]]))
    final = fits[5]
    count = final['class_count'].astype(np.float64)
    fit = dict(theta=final['theta'], var=final['var'], epsilon=final['epsilon'], class_count=count, class_prior=count / count.sum(),
               n_features=X.shape[1])
    return classes, scores, fit


def as_sklearn_logistic(fit, classes):
    """A scikit-learn LogisticRegression(solver='liblinear', penalty='l1') holding the fitted weights (what the reference pickles
    for -c LR).  multi_class stays at its default, so predict_proba is expit(decision_function), the form model_io scores."""
    from sklearn.linear_model import LogisticRegression
    m = LogisticRegression(solver='liblinear', penalty='l1')
    m.n_features_in_ = int(fit['n_features'])
    m.classes_ = np.array(classes)
    m.coef_ = np.asarray(fit['coef'], dtype=np.float64).reshape(1, -1)
    m.intercept_ = np.array([fit['intercept']], dtype=np.float64).reshape(1)
    m.n_iter_ = np.array([fit['n_iter']], dtype=np.int32)
    return m


def as_sklearn_gnb(fit, classes):
    """A scikit-learn GaussianNB holding the fitted means, variances (smoothing included) and priors (-c NBC)."""
    from sklearn.naive_bayes import GaussianNB
    m = GaussianNB()
    m.n_features_in_ = int(fit['n_features'])
    m.classes_ = np.array(classes)
    m.theta_ = np.asarray(fit['theta'], dtype=np.float64).reshape(2, -1)
    m.var_ = np.asarray(fit['var'], dtype=np.float64).reshape(2, -1)
    m.class_count_ = np.asarray(fit['class_count'], dtype=np.float64)
    m.class_prior_ = np.asarray(fit['class_prior'], dtype=np.float64)
    m.epsilon_ = float(fit['epsilon'])
    return m


def _classifiers():
    """What differs between the classifiers of `-c`, by name: the fit, the scikit-learn estimator of a fit (fit, classes, rows it was
    fitted on) and the arrays of a fit in the neutral `.npz` (model_io reads them).  Built when asked for, so that a fit_*_on_gpu
    replaced in this module is the one that runs."""
    return {
        'NN': dict(fit=fit_nn_on_gpu, as_sklearn=as_sklearn_estimator,
                   npz=lambda fit: {'W1': fit['W1'], 'b1': fit['b1'], 'W2': fit['W2'], 'b2': np.array([fit['b2']])}),
        'RF': dict(fit=fit_rf_on_gpu, as_sklearn=lambda fit, classes, n: as_sklearn_forest(fit, classes),
                   npz=lambda fit: dict({name: fit[name] for name in ('tree_off', 'left', 'right', 'feature', 'threshold', 'value')},
                                        n_features=np.array([fit['n_features']]))),
        'SVM': dict(fit=fit_svm_on_gpu, as_sklearn=lambda fit, classes, n: as_sklearn_svc(fit, classes),
                    npz=lambda fit: {'sv': fit['sv'], 'dual_coef': fit['dual_coef'],
                                     'svm_params': np.array([fit['gamma'], fit['intercept'], fit['probA'], fit['probB']], dtype=np.float64)}),
        'LR': dict(fit=fit_lr_on_gpu, as_sklearn=lambda fit, classes, n: as_sklearn_logistic(fit, classes),
                   npz=lambda fit: {'lr_coef': np.asarray(fit['coef'], dtype=np.float64),
                                    'lr_intercept': np.array([fit['intercept']], dtype=np.float64)}),
        'NBC': dict(fit=fit_nb_on_gpu, as_sklearn=lambda fit, classes, n: as_sklearn_gnb(fit, classes),
                    npz=lambda fit: {'nb_theta': fit['theta'], 'nb_var': fit['var'], 'nb_prior': fit['class_prior']}),
    }


def write_models(models, classes_of, n_of, modelfile, classifier='NN'):
    clf = _classifiers()[classifier]
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    if have_sklearn:
        out = {key: clf['as_sklearn'](fit, classes_of[key], n_of.get(key)) for key, fit in models.items()}    # (n: the NN's t_ only)
        with open(modelfile, 'wb') as modfi:
            pickle.dump(out, modfi)
        return out
    arrays = {'__is_dict__': np.array([1])}
    for key, fit in models.items():
        for name, array in clf['npz'](fit).items():
            arrays[key + '.' + name] = array
        arrays[key + '.classes'] = np.array(classes_of[key])
    with open(modelfile, 'wb') as modfi:
        np.savez(modfi, **arrays)
    return models


def train_classifier(signals, groups, modelfile, classifier='NN', plot=False, device=None):
    if plot:
        raise NotImplementedError('--plot_training is not supported (it raises NameError in the reference: the import '
                                  'of plotlib is commented out, train_model.py:3,:108)')
    if classifier not in _classifiers():
        raise ValueError('unknown classifier ' + str(classifier))
    models, classes_of, n_of = {}, {}, {}
    for twobase_model in signals:
        balance = balanced_arrays if _has_array_leaves(signals[twobase_model]) else balanced_rows
        labs, sigs, grps = balance(signals[twobase_model], groups[twobase_model])
        print(_shown(labs))
        print(_shown(sigs))
        print(_shown(grps))
        classes, scores, fit = _classifiers()[classifier]['fit'](labs, sigs, grps, bool(groups), device=device)
        print('%s %s model scores: %s' % (classifier, twobase_model, ','.join([str(s) for s in scores])))
        print('Cross validation accuracy: %0.2f (+/- %0.2f)' % (scores.mean(), scores.std() * 2))
        models[twobase_model], classes_of[twobase_model], n_of[twobase_model] = fit, classes, len(labs)
    return write_models(models, classes_of, n_of, modelfile, classifier)
