"""Small problems for the NBC fit kernel (k7_nb_fit, csrc/mc_simple_fit.hip), one per edge of the kernel: a seeded generator and a named
table.  A case is the smallest problem that still reaches the edge it names.  The yardstick is EXACT: the two-pass means and variances
of the definition in `fractions.Fraction` over the float64 inputs (`exact(case)`, computed once per process); tests/test_nb_fit_cases.py
checks on the CPU that every case reaches its edge and that the NumPy oracle (tests/nb_fit_oracle.py) alone meets the bound below,
tests/test_gpu_nb_fit_edges.py holds the kernel to the same bound, element by element.

What the kernel does with a case (read from mc_simple_fit.hip, restated here so that the CPU file can check the table):
  * one workgroup of BT = 512 lanes per job; the job's rows are grouped classes_[0] first (stable), row t is class 0 iff t < n0;
  * lane `tid` adds its rows t = tid + 512 r in order (one partial sum per class and one for all rows), then a butterfly over the
    64 lanes of a wave (6 steps), then thread f adds the 8 waves' sums in order;
  * means first, then the centred squares against the class mean (a second pass), then the job-wide variance against the job-wide
    mean (a third), epsilon = var_smoothing * max_f var_f, var = var + epsilon;
  * the held-out rows' joint log-likelihood sums run as numpy's pairwise_sum does: in order below 8 terms, eight partial sums from
    8 on (np_sum) -- hence the widths 7, 8, 9, 15, 16, 17; class 1 is predicted iff jll[1] > jll[0]: ties go to class 0.

THE BOUND (derived, not tuned).  u = 2^-53.  A class (or the whole job) of m rows, contiguous in t, gives a lane at most ceil(m / 512)
of its rows, so a sum passes every term through at most
    K(m) = ceil(m / 512) + 6 + 8
additions: |fl(sum x) - sum x| <= g(K) sum |x|, g(k) = k u / (1 - k u) (Higham, Accuracy and Stability, ch. 4: any order of
addition, k the longest chain).  The division by m rounds once more.  A term of the second pass rounds three more times: x - mean
once, and the square carries that one twice and adds its own.  Hence
    K'(m) = K(m) + 4     (19 up to 512 rows of a class, 20 up to 1024, 21 up to 1536)
and, with M the exact mean, V the exact (two-pass, population) variance and A the exact mean of |x| of a class and column:
    |theta - M| <= T := g(K') A                                                                   (K + 1 would do; one constant is kept)
    the centred sum is taken about theta, not M: sum (x - theta)^2 = sum (x - M)^2 + m (theta - M)^2 exactly, so
    |v - V| <= W := g(K') (V + T^2) + T^2             for v the kernel's variance before smoothing  ("the mean's term" is T^2)
    |epsilon - E| <= g(1) (E + s max_f W_f) + s max_f W_f   for E = s max_f V_f over ALL the job's rows, s = var_smoothing, K' of l
The kernel reports var = fl(v + epsilon) only, so the tests take var - epsilon exactly (in Fractions) and add the rounding of that one
addition, u var; var itself is held to W + (the bound of epsilon) + 2^-52 (V + E).  A one-pass variance (sum x^2 / m - M^2) misses W by
ten orders of magnitude on the `far_mean` column (1e8 + N(0, 1e-3): it is wrong by about u 1e16 = 1); a tolerance relative to the
largest variance of all columns, as tests/test_gpu_simple_fit.py has it, would let a column of variance 1e-8 be wrong by 1e-3 of itself.

The NumPy oracle adds a class's rows one after another (up to 1024 roundings in the worst case, about sqrt(m) of them typically): it
meets the bound on every case here, by a margin tests/test_nb_fit_cases.py states; that is a condition on the seeds.

Held-out rows: N_VAL rows of the same generator after the training rows.  No held-out row of any case but `tie` has a joint
log-likelihood gap inside the band of tests/test_gpu_simple_fit.py (1e-9 (1 + max |jll|)): the device must count exactly what the
oracle counts.  In `tie` every held-out row has jll[0] == jll[1] bit for bit (all the arithmetic is exact): class 0."""
import functools
from fractions import Fraction

import numpy as np

from tests import nb_fit_oracle as no

BT = 512                   # lanes of k7_nb_fit's workgroup
N_VAL = 64                 # held-out rows of a single-job case
U = Fraction(1, 2 ** 53)
VAR_SMOOTHING = 1e-9


def chain(m):
    """K(m): the longest chain of additions a term of a sum over m rows (contiguous in t) goes through."""
    return -(-m // BT) + 6 + 8


def k_prime(m):
    return chain(m) + 4


def g(k):
    return k * U / (1 - k * U)


def _case(name, edge, l, n0, d, kind='normal', seed=1, **expect):
    return dict(name=name, edge=edge, l=l, n0=n0, d=d, kind=kind, seed=seed, expect=expect)


# the multi-job call of the LR table: training sizes and held-out sizes (odd offsets, an empty and a long held-out set)
MULTI_L, MULTI_VA = (2, 65, 513, 3), (0, 1, 513, 64)


def _table():
    t = []
    # ---- training sizes on the lane, wave and block boundaries, the class split at either end and on the block edge ----
    for l in (2, 511, 512, 513, 1025):
        for n0 in sorted({1, l - 1, 512, 513}):
            if 1 <= n0 <= l - 1:
                t.append(_case('rows_%d_n0_%d' % (l, n0), 'rows', l, n0, 3, n1=l - n0,
                               one_row_class=n0 == 1 or l - n0 == 1, strides0=-(-n0 // BT), strides1=-(-(l - n0) // BT)))
    # ---- widths around np_sum's switch at 8 terms, and the largest ----
    for d in (1, 7, 8, 9, 15, 16, 17, 64):
        t.append(_case('width_%d' % d, 'width', 130, 61, d, pairwise=d >= 8, tail=d % 8 if d >= 8 else d))
    # ---- columns a careless variance gets wrong ----
    # (the constant columns stay short: adding one constant 250 times one after another, as the NumPy oracle does, rounds the same way
    # every time and is off by 37 u where the kernel's longest chain allows 19 u; at 61 and 69 rows it stays within 12 u)
    t.append(_case('const_col', 'column', 130, 61, 3, 'const_col', zero_var=((0, 0), (1, 0))))
    t.append(_case('const_in_class', 'column', 130, 61, 3, 'const_in_class', zero_var=((0, 0),)))
    t.append(_case('far_mean', 'column', 600, 250, 2, 'far_mean'))
    t.append(_case('var_scales', 'column', 600, 250, 2, 'var_scales'))
    t.append(_case('far_mean_one_row_class', 'column', 513, 1, 2, 'far_mean', zero_var=((0, 0), (0, 1))))
    # ---- exactly equal joint log-likelihoods: ties go to class 0 ----
    t.append(_case('tie', 'tie', 600, 300, 2, 'tie', seed=2))
    return {c['name']: c for c in t}


CASES = _table()
MULTI = _case('multi_job', 'jobs', sum(MULTI_L), 0, 3, seed=4)


def columns(kind, rng, n, d, y):
    """n rows of d columns for the labels y."""
    X = rng.normal(size=(n, d)) * np.linspace(0.5, 3.0, d)
    X[:, 0] += np.where(y == 1, 1.0, -1.0) * 0.5
    if kind == 'const_col':
        X[:, 0] = 7.3
    elif kind == 'const_in_class':
        X[y == 0, 0] = 0.1
    elif kind == 'far_mean':
        X[:, 0] = 1e8 + rng.normal(size=n) * 1e-3 + np.where(y == 1, 2e-3, 0.0)
        X[:, 1] = rng.normal(size=n) * 3.0
    elif kind == 'var_scales':
        X[:, 0] = rng.normal(size=n) * 1e-4 + np.where(y == 1, 2e-4, 0.0)
        X[:, 1] = rng.normal(size=n) * 3.0 + np.where(y == 1, 1.0, 0.0)
    elif kind != 'normal':
        raise ValueError(kind)
    return np.ascontiguousarray(X)


def problem(case):
    """-> X [l + N_VAL, d], y, jobs [(training rows in a seeded order, held-out rows)]: exactly n0 rows of class 0 among the first l,
    scattered, so that the entry point's grouping is part of what is tested."""
    rng = np.random.default_rng([case['seed'], case['l'], case['d']])
    l, n0, d = case['l'], case['n0'], case['d']
    if case['kind'] == 'tie':
        # two points per class, mirrored: class 0 at -3 and -1, class 1 at 1 and 3 (column 1: the mirror image, doubled); every sum
        # is a sum of small integers, so means, variances and the two classes' log-likelihoods at x = 0 are exact and equal
        assert l % 4 == 0 and n0 * 2 == l and d == 2
        y = (np.arange(l) % 2).astype(np.uint8)
        a = np.where(y == 0, np.where(np.arange(l) % 4 == 0, -3.0, -1.0), np.where(np.arange(l) % 4 == 1, 1.0, 3.0))
        X = np.stack([a, -2.0 * a], axis=1)
        Xv = np.zeros((N_VAL, 2))
        yv = (np.arange(N_VAL) % 3 == 0).astype(np.uint8)
        X, y = np.concatenate([X, Xv]), np.concatenate([y, yv])
    else:
        y = np.ones(l + N_VAL, dtype=np.uint8)
        y[rng.permutation(l)[:n0]] = 0
        y[l:] = rng.integers(0, 2, N_VAL)
        X = columns(case['kind'], rng, l + N_VAL, d, y)
    return np.ascontiguousarray(X), y, [(rng.permutation(l), np.arange(l, l + N_VAL))]


def multi_problem():
    """The multi-job call: jobs of l = MULTI_L training rows and MULTI_VA held-out rows, cut one after another from one matrix."""
    rng = np.random.default_rng([MULTI['seed'], 99])
    n = sum(MULTI_L) + sum(MULTI_VA)
    y = rng.integers(0, 2, n).astype(np.uint8)
    jobs, at = [], 0
    for l, nv in zip(MULTI_L, MULTI_VA):
        y[at], y[at + 1] = 0, 1                              # both classes in every job
        jobs.append((at + rng.permutation(l), np.arange(at + l, at + l + nv)))
        at += l + nv
    return columns('normal', rng, n, MULTI['d'], y), y, jobs


def _frac_col(x):
    return [Fraction(float(v)) for v in x]


def exact_fit(X, y, train, var_smoothing=VAR_SMOOTHING):
    """The definition in exact rationals on the training rows `train` -> dict of [2][d] lists of Fractions M (means), V (two-pass
    population variances), A (means of |x|), of [d] lists Vall, Aall (all rows), of E (epsilon), count, and of the bounds T, W
    ([2][d]), eps_tol (module docstring)."""
    Xt, yt = X[train], y[train]
    d = X.shape[1]
    out = dict(M=[[], []], V=[[], []], A=[[], []], T=[[], []], W=[[], []], Vall=[], Wall=[], count=[int((yt == 0).sum()), int((yt == 1).sum())])

    def stats(col):
        m = len(col)
        mean = sum(col) / m
        return mean, sum((x - mean) ** 2 for x in col) / m, sum(abs(x) for x in col) / m, g(k_prime(m))

    def bounds(V, A, gk):
        T = gk * A
        return T, gk * (V + T * T) + T * T

    for f in range(d):
        col = _frac_col(Xt[:, f])
        for c in (0, 1):
            M, V, A, gk = stats([x for x, lab in zip(col, yt) if lab == c])
            T, W = bounds(V, A, gk)
            for k, v in zip('MVATW', (M, V, A, T, W)):
                out[k][c].append(v)
        M, V, A, gk = stats(col)
        out['Vall'].append(V)
        out['Wall'].append(bounds(V, A, gk)[1])
    s = Fraction(float(var_smoothing))
    out['E'] = s * max(out['Vall'])
    slack = s * max(out['Wall'])
    out['eps_tol'] = g(1) * (out['E'] + slack) + slack
    return out


@functools.lru_cache(maxsize=None)
def _exact_by_name(name):
    if name == MULTI['name']:
        X, y, jobs = multi_problem()
    else:
        X, y, jobs = problem(CASES[name])
    return [exact_fit(X, y, tr) for tr, _ in jobs]


def exact(case):
    """The exact fits of the case's jobs, computed once and shared: do not write into them."""
    return _exact_by_name(case['name'])


def check_fit(got, ex):
    """Hold a fit (dict theta [2, d], var [2, d], epsilon, class_count) to the exact one within the derived bounds -> a list of the
    misses as strings (empty: the fit passes), and the largest used fraction of a bound."""
    bad, worst = [], 0.0

    def hold(what, err, tol):
        nonlocal worst
        if tol == 0:
            if err != 0:
                bad.append('%s: off by %.3e where the bound is 0' % (what, float(err)))
            return
        worst = max(worst, float(err / tol))
        if err > tol:
            bad.append('%s: off by %.3e, bound %.3e' % (what, float(err), float(tol)))

    eps = Fraction(float(got['epsilon']))
    hold('epsilon', abs(eps - ex['E']), ex['eps_tol'])
    if list(np.asarray(got['class_count']).tolist()) != ex['count']:
        bad.append('class_count %s, not %s' % (got['class_count'], ex['count']))
    d = len(ex['Vall'])
    for c in (0, 1):
        for f in range(d):
            th, vr = Fraction(float(got['theta'][c][f])), Fraction(float(got['var'][c][f]))
            hold('theta[%d][%d]' % (c, f), abs(th - ex['M'][c][f]), ex['T'][c][f])
            hold('var - epsilon [%d][%d]' % (c, f), abs(vr - eps - ex['V'][c][f]), ex['W'][c][f] + U * vr)
            hold('var[%d][%d]' % (c, f), abs(vr - (ex['V'][c][f] + ex['E'])), ex['W'][c][f] + ex['eps_tol'] + 2 * U * (ex['V'][c][f] + ex['E']))
    return bad, worst


def band_rows(fit, X, va):
    """Held-out rows whose joint log-likelihood gap lies inside the band of tests/test_gpu_simple_fit.py."""
    if not len(va):
        return 0
    jll = no.joint_log_likelihood(fit, X[va])
    return int((np.abs(jll[:, 1] - jll[:, 0]) < 1e-9 * (1 + np.abs(jll).max(axis=1))).sum())


assert k_prime(512) == 19 and k_prime(513) == 20 and k_prime(1025) == 21
