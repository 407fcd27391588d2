"""CPU restatement (numpy) of the `--train -c SVM` fit (mc_svm_fit, k6_svm_fit): what scikit-learn's SVC(kernel='rbf',
probability=True) computes through libsvm, as train_model.fit_svm_on_gpu splits it into solves.  TEST INFRASTRUCTURE: the yardstick
the device is held to, never the product.

* gamma='scale': 1 / (d X.var()) on the rows a fit is given (1.0 if the variance is 0), as SVC.fit resolves it.
* The solve: libsvm's Solver without shrinking -- G = -1, alpha = 0; i = argmax -y G over I_up, j by the second-order rule over
  I_low (tau = 1e-12), stop when Gmax + Gmax2 < eps; libsvm's two clipping cases; rho the mean of y G over the free alphas or the
  midpoint of the bounds.  Ties go to the lowest index.  Kernel values in fp64, exp(-gamma sum_f (x_f - x'_f)^2), f in order.
* Platt scaling (svm_binary_svc_probability): the rows grouped by class (classes_[0] first, label +1), shuffled with
  perm[i] <-> perm[i + bounded_rand_int(l - i)] (std::mt19937 and Lemire's bounded draw, scikit-learn's newrand.h), five folds of
  positions, a solve on each fold's complement (or dec = +-1 when it holds one class), then sigmoid_train in sequential Python floats.
"""
import math

import numpy as np

from tests import svm_oracle

TAU = 1e-12


def gamma_of(X):
    X = np.asarray(X, dtype=np.float64)
    var = X.var()
    return 1.0 / (X.shape[1] * var) if var != 0 else 1.0


def permutation(l, seed):
    """libsvm's shuffle, one draw at a time."""
    mt = np.random.MT19937()
    mt._legacy_seeding(int(seed))
    perm = list(range(l))
    for i in range(l):
        rng = l - i
        x = int(mt.random_raw())
        m = x * rng
        if (m & 0xFFFFFFFF) < rng:
            t = (-rng) & 0xFFFFFFFF
            if t >= rng:
                t -= rng
                if t >= rng:
                    t %= rng
            while (m & 0xFFFFFFFF) < t:
                x = int(mt.random_raw())
                m = x * rng
        j = i + (m >> 32)
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm, dtype=np.int64)


def kernel_rows(A, B, gamma):
    """K[a, b] = exp(-gamma sum_f (A[a, f] - B[b, f])^2), the differences squared and added feature by feature."""
    d2 = np.zeros((len(A), len(B)))
    for f in range(A.shape[1]):
        t = A[:, f][:, None] - B[:, f][None, :]
        d2 = d2 + t * t
    return np.exp(-gamma * d2)


CLIPS = ('diff_pos_aj_below_0', 'diff_neg_ai_below_0', 'diff_pos_ai_above_C', 'diff_neg_aj_above_C',
         'sum_big_ai_above_C', 'sum_small_aj_below_0', 'sum_big_aj_above_C', 'sum_small_ai_below_0')
SMO_MUTANTS = ('ties_to_highest_index',) + tuple('skip_' + c for c in CLIPS) + ('tau_ignored', 'rho_midpoint_as_mean')


def _ulp_signs(d2, seed):
    """+1 / -1 per entry, a fixed function of the entry's bits and the seed (an exp that is one ulp off is off the same way
    wherever its argument is the same: equal squared distances keep equal kernel values)."""
    h = np.ascontiguousarray(d2).view(np.uint64) ^ np.uint64(0x9E3779B97F4A7C15 * (2 * int(seed) + 1) % 2 ** 64)
    h = h * np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(31)
    h = h * np.uint64(0x94D049BB133111EB)
    return np.where((h >> np.uint64(40)) & np.uint64(1), 1.0, -1.0)


def _first_max(v, last=False):
    return len(v) - 1 - int(np.argmax(v[::-1])) if last else int(np.argmax(v))


def _gap(v, k):
    """(v[k] minus the largest other entry, that entry's index): (inf, -1) without a rival."""
    rest = v.copy()
    rest[k] = -np.inf
    r = int(np.argmax(rest))
    if rest[r] == -np.inf:
        return math.inf, -1
    return float(v[k] - rest[r]), r


def smo(X, ys, gamma, C=1.0, eps=1e-3, max_iter=None, trace=None, mutate=None, wobble=None):
    """One solve on the rows X (in solve order) with labels ys in {+1, -1}.  -> dict(alpha, rho, n_iter, status).
    trace=: a dict that gets a Counter 'branches' -- the eight clipping branches (CLIPS, named by libsvm's tests: the sign of
    diff = ai - aj for unequal labels, sum = ai + aj against C for equal ones, then the bound crossed), tau_select (a candidate j
    with quad <= 0, an exact duplicate of row i) and tau_update, rho_mean / rho_midpoint, and the loop's three exits exit_max_iter,
    exit_no_up (I_up empty) and exit_converged (Gmax + Gmax2 < eps, or no candidate) -- and the lists 'gap_i' and 'gap_j': per
    selection the chosen candidate's value minus the runner-up's (0: an exact tie, won by the lowest index), and the list 'picks' of
    (i, runner-up of i, j, runner-up of j, Gmax = -y_i G_i) per selection (-1: no rival).
    mutate=: one of SMO_MUTANTS, a defect on purpose.  wobble=: a seed; every kernel value other than an exact 1 is multiplied by
    1 + 2^-52 or 1 - 2^-52 (_ulp_signs): an exp one ulp off.  With the defaults no returned bit changes."""
    if mutate not in (None,) + SMO_MUTANTS:
        raise ValueError('smo: mutate is one of SMO_MUTANTS')
    import collections
    X = np.asarray(X, dtype=np.float64)
    ys = np.asarray(ys, dtype=np.float64)
    l = len(ys)
    if max_iter is None:
        max_iter = max(10 ** 7, 100 * l)
    cols = [np.ascontiguousarray(X[:, f]) for f in range(X.shape[1])]
    seen = collections.Counter()
    gap_i, gap_j, picks = [], [], []
    last = mutate == 'ties_to_highest_index'

    def row(i):
        d2 = np.zeros(l)
        for c in cols:
            t = c[i] - c
            d2 = d2 + t * t
        k = np.exp(-gamma * d2)
        if wobble is not None:
            k = np.where(d2 == 0, k, k * (1.0 + _ulp_signs(d2, wobble) * 2.0 ** -52))
        return k

    def clip(name, test):
        """libsvm's `if (test)` of the branch `name`: counted, and not taken by the mutant that skips it."""
        if test:
            seen[name] += 1
        return test and mutate != 'skip_' + name

    alpha = np.zeros(l)
    G = -np.ones(l)
    it, status = 0, 0
    pos = ys > 0
    while True:
        if it >= max_iter:
            status = 1
            seen['exit_max_iter'] += 1
            break
        up = np.where(pos, alpha < C, alpha > 0)
        if not up.any():
            seen['exit_no_up'] += 1
            break
        v = np.where(up, -ys * G, -np.inf)
        i = _first_max(v, last)                               # (the first of equals)
        Gmax = v[i]
        Ki = row(i)
        low = np.where(pos, alpha > 0, alpha < C)
        yg = ys * G
        Gmax2 = yg[low].max() if low.any() else -np.inf
        gd = Gmax + yg
        cand = low & (gd > 0)
        quad = 1.0 + 1.0 - 2.0 * Ki
        with np.errstate(divide='ignore', invalid='ignore'):
            obj = -(gd * gd) / (quad if mutate == 'tau_ignored' else np.where(quad > 0, quad, TAU))
        if Gmax + Gmax2 < eps or not cand.any():
            seen['exit_converged'] += 1
            break
        score = np.where(cand, -obj, -np.inf)
        if mutate == 'tau_ignored':
            score = np.where(np.isnan(score), -np.inf, score)
        j = _first_max(score, last)
        if trace is not None:
            (gi, ri), (gj, rj) = _gap(v, i), _gap(score, j)
            gap_i.append(gi)
            gap_j.append(gj)
            picks.append((i, ri, j, rj, float(Gmax)))
            if (cand & (quad <= 0)).any():
                seen['tau_select'] += 1
        it += 1
        yi, yj = ys[i], ys[j]
        ai0, aj0, Gi, Gj = alpha[i], alpha[j], G[i], G[j]
        Qij = (yi * yj) * Ki[j]
        ai, aj = ai0, aj0
        if yi != yj:
            q = 1.0 + 1.0 + 2.0 * Qij
            if q <= 0:
                seen['tau_update'] += 1
            q = q if q > 0 or mutate == 'tau_ignored' else TAU
            with np.errstate(divide='ignore', invalid='ignore'):
                delta = np.float64(-Gi - Gj) / q
            diff = ai - aj
            ai += delta
            aj += delta
            if diff > 0:
                if clip(CLIPS[0], aj < 0):
                    aj, ai = 0.0, diff
            elif clip(CLIPS[1], ai < 0):
                ai, aj = 0.0, -diff
            if diff > C - C:
                if clip(CLIPS[2], ai > C):
                    ai, aj = C, C - diff
            elif clip(CLIPS[3], aj > C):
                aj, ai = C, C + diff
        else:
            q = 1.0 + 1.0 - 2.0 * Qij
            if q <= 0:
                seen['tau_update'] += 1
            q = q if q > 0 or mutate == 'tau_ignored' else TAU
            with np.errstate(divide='ignore', invalid='ignore'):
                delta = np.float64(Gi - Gj) / q
            s = ai + aj
            ai -= delta
            aj += delta
            if s > C:
                if clip(CLIPS[4], ai > C):
                    ai, aj = C, s - C
            elif clip(CLIPS[5], aj < 0):
                aj, ai = 0.0, s
            if s > C:
                if clip(CLIPS[6], aj > C):
                    aj, ai = C, s - C
            elif clip(CLIPS[7], ai < 0):
                ai, aj = 0.0, s
        dai, daj = ai - ai0, aj - aj0
        Kj = row(j)
        G = G + (((yi * ys) * Ki) * dai + ((yj * ys) * Kj) * daj)
        alpha[i], alpha[j] = ai, aj
    free = (alpha > 0) & (alpha < C)
    seen['rho_mean' if free.any() else 'rho_midpoint'] += 1
    if mutate == 'rho_midpoint_as_mean' and not free.any():
        rho = float((ys * G).mean())
    else:
        rho = rho_of(alpha, ys, G, C)
    if trace is not None:
        trace['branches'], trace['gap_i'], trace['gap_j'], trace['picks'] = seen, gap_i, gap_j, picks
    return dict(alpha=alpha, rho=rho, n_iter=it, status=status)


def rho_of(alpha, ys, G, C=1.0):
    yG = ys * G
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        return float(yG[free].mean())
    ub = np.concatenate([yG[upper & (ys < 0)], yG[lower & (ys > 0)], [np.inf]]).min()
    lb = np.concatenate([yG[upper & (ys > 0)], yG[lower & (ys < 0)], [-np.inf]]).max()
    return float((ub + lb) / 2)


def gradient(X, ys, alpha, gamma, chunk=2048):
    """G = Q alpha - 1 recomputed from alpha (Q_ts = y_t y_s K_ts)."""
    X = np.asarray(X, dtype=np.float64)
    sv = alpha > 0
    c = (ys * alpha)[sv]
    G = np.empty(len(ys))
    for a in range(0, len(ys), chunk):
        G[a:a + chunk] = ys[a:a + chunk] * (kernel_rows(X[a:a + chunk], X[sv], gamma) @ c) - 1.0
    return G


def kkt_violation(X, ys, alpha, gamma, C=1.0):
    """Gmax + Gmax2 of a solution, G recomputed: libsvm stops below eps."""
    G = gradient(X, ys, alpha, gamma)
    pos = ys > 0
    up = np.where(pos, alpha < C, alpha > 0)
    low = np.where(pos, alpha > 0, alpha < C)
    gmax = (-ys * G)[up].max() if up.any() else -np.inf
    gmax2 = (ys * G)[low].max() if low.any() else -np.inf
    return max(0.0, float(gmax + gmax2))


def dual_objective(X, coef, gamma, chunk=2048):
    """0.5 c^T K c - sum |c| over the support vectors X with dual coefficients c = y alpha."""
    X = np.asarray(X, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64).reshape(-1)
    q = 0.0
    for a in range(0, len(c), chunk):
        q += float(c[a:a + chunk] @ (kernel_rows(X[a:a + chunk], X, gamma) @ c))
    return 0.5 * q - float(np.abs(c).sum())


SIGMOID_MUTANTS = ('no_backtracking', 'targets_swapped')


def sigmoid_train(dec, labels, trace=None, order=None, mutate=None):
    """libsvm's sigmoid_train, sequential Python floats.  labels: +1 / -1 (> 0 counts as prior1).  -> (A, B).
    trace=: a dict that gets 'halvings' (a list: the halvings of every Newton iteration that searched) and 'exit', one of
    'gradient_at_entry' (the gradient below eps before any step: the starting point is returned), 'gradient', 'min_step' and
    'max_iter'.  order='device': the sums in k6_svm_sigmoid's order (csrc/mc_svm_fit.hip: `reduce`) -- lane tid of ST = 1024 adds
    its values k = tid + ST r in order from 0.0, s += shfl_xor(s, o) for o = 32 .. 1 over a wave, the 16 waves' sums in order from
    0.0, and sigma added to h11 and h22 after the sum; it shows that a case does not hang on the order, it is not a yardstick.
    mutate=: one of SIGMOID_MUTANTS, a defect on purpose.  With the defaults no returned bit changes."""
    if order not in (None, 'device') or mutate not in (None,) + SIGMOID_MUTANTS:
        raise ValueError("sigmoid_train: order is None or 'device', mutate one of SIGMOID_MUTANTS")
    dec = [float(v) for v in dec]
    lab = [float(v) for v in labels]
    l = len(dec)
    prior1 = float(sum(1 for v in lab if v > 0))
    prior0 = float(l) - prior1
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hiTarget = (prior1 + 1.0) / (prior1 + 2.0)
    loTarget = 1 / (prior0 + 2.0)
    if mutate == 'targets_swapped':
        t = [loTarget if v > 0 else hiTarget for v in lab]
    else:
        t = [hiTarget if v > 0 else loTarget for v in lab]
    A, B = 0.0, math.log((prior0 + 1.0) / (prior1 + 1.0))
    halvings, leave = [], 'max_iter'

    def total(start, terms):
        if order == 'device':
            from tests.lr_fit_oracle import device_sum
            s = 0.0
            for w in device_sum(np.asarray(terms, dtype=np.float64), 1024):
                s = s + float(w)
            return start + s
        for v in terms:
            start += v
        return start

    def fun(A, B):
        terms = []
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                terms.append(t[i] * fApB + math.log(1 + math.exp(-fApB)))
            else:
                terms.append((t[i] - 1) * fApB + math.log(1 + math.exp(fApB)))
        return total(0.0, terms)

    fval = fun(A, B)
    for it in range(max_iter):
        sums = [[], [], [], [], []]
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                p = math.exp(-fApB) / (1.0 + math.exp(-fApB))
                q = 1.0 / (1.0 + math.exp(-fApB))
            else:
                p = 1.0 / (1.0 + math.exp(fApB))
                q = math.exp(fApB) / (1.0 + math.exp(fApB))
            d2 = p * q
            d1 = t[i] - p
            for k, v in enumerate((dec[i] * dec[i] * d2, d2, dec[i] * d2, dec[i] * d1, d1)):
                sums[k].append(v)
        h11, h22, h21, g1, g2 = (total(start, terms) for start, terms in zip((sigma, sigma, 0.0, 0.0, 0.0), sums))
        if abs(g1) < eps and abs(g2) < eps:
            leave = 'gradient_at_entry' if it == 0 else 'gradient'
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        stepsize = 1
        n_half = 0
        while stepsize >= min_step:
            newA, newB = A + stepsize * dA, B + stepsize * dB
            newf = fun(newA, newB)
            if newf < fval + 0.0001 * stepsize * gd or mutate == 'no_backtracking':
                A, B, fval = newA, newB, newf
                break
            stepsize = stepsize / 2.0
            n_half += 1
        halvings.append(n_half)
        if stepsize < min_step:
            leave = 'min_step'
            break
    if trace is not None:
        trace['halvings'], trace['exit'] = halvings, leave
    return A, B


def grouped(rows, y, first):
    rows = np.asarray(rows)
    return np.concatenate([rows[y[rows] == first], rows[y[rows] != first]])


def solve_job(X, y, train, val, gamma):
    """A solve on rows `train` (solve order: the first row's class is +1) and the decision values of rows `val`, turned so that
    > 0 means class 0.  -> dict(alpha, rho, n_iter, status, val_dec, val_correct)."""
    ys = np.where(y[train] == y[train[0]], 1.0, -1.0)
    s = smo(X[train], ys, gamma)
    sign = 1.0 if y[train[0]] == 0 else -1.0
    sv = s['alpha'] > 0
    dec = sign * svm_oracle.decision(X[train][sv], (ys * s['alpha'])[sv], gamma, -s['rho'], X[val]) if len(val) else np.zeros(0)
    s.update(val_dec=dec, val_correct=int((np.where(dec > 0, 0, 1) == y[val]).sum()))
    return s


def platt_seed(seed):
    return int(seed % (2 ** 31 - 1))


def fit_submodel(X, y, jobs, seed):
    """The whole -c SVM fit of a sub-model: jobs = train_model.cv_jobs' six (train, val) jobs, seed = the final job's seed.
    -> dict(cv=[solve of fold f or None], gammas, final (solve), order, perm, platt_dec, A, B, fit: as train_model.fit_svm_on_gpu's)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y)
    cv, gammas = [], []
    for tr, va in jobs[:5]:
        g = gamma_of(X[tr])
        gammas.append(g)
        cv.append(solve_job(X, y, grouped(tr, y, 0), va, g) if len(set(y[tr].tolist())) == 2 else None)
    order = grouped(np.arange(len(y)), y, 0)
    gamma = gamma_of(X)
    final = solve_job(X, y, order, np.zeros(0, dtype=np.int64), gamma)
    l = len(order)
    perm = permutation(l, platt_seed(seed))
    dec = np.zeros(l)
    platt = []
    for f in range(5):
        begin, end = f * l // 5, (f + 1) * l // 5
        comp = order[np.concatenate([perm[:begin], perm[end:]])]
        held = perm[begin:end]
        labs = set(y[comp].tolist())
        if len(labs) == 2:
            s = solve_job(X, y, grouped(comp, y, 1), order[held], gamma)
            dec[held] = s['val_dec']
            platt.append(s)
        else:
            dec[held] = 0.0 if not labs else (1.0 if labs == {0} else -1.0)
            platt.append(None)
    labels = np.where(y[order] == 0, 1.0, -1.0)
    A, B = sigmoid_train(dec, labels)
    sv = final['alpha'] > 0
    support = order[sv]
    fit = dict(support=support.astype(np.int32), sv=X[support], dual_coef=(labels * final['alpha'])[sv], intercept=-final['rho'],
               gamma=gamma, probA=A, probB=B, n_support=np.array([(y[support] == 0).sum(), (y[support] == 1).sum()], np.int32),
               n_iter=final['n_iter'], status=final['status'], n_samples=len(y), n_features=X.shape[1])
    return dict(cv=cv, gammas=gammas + [gamma], final=final, order=order, perm=perm, platt=platt, platt_dec=dec, A=A, B=B, fit=fit)
