"""Small problems for the SVM fit kernels (k6_svm_fit, k6_svm_val, k6_svm_sigmoid, csrc/mc_svm_fit.hip): SOLVE cases on the lane, wave
and block boundaries of the solver's row loops, with exact ties, at both ends of C and at capped iterates, and SIGMOID cases for the
Platt solver.  A case is a seeded generator call plus parameters; the yardstick is tests/svm_fit_oracle.py (smo, sigmoid_train) on the
same rows and parameters (`oracle(case)`, computed once per process).  tests/test_svm_fit_cases.py checks on the CPU that every case
reaches what it names, that an exp one ulp off does not change the way a solve goes, and that a kernel wrong in a branch would fail
the case that holds that branch; tests/test_gpu_svm_fit_edges.py holds the kernels to the table.

What the kernels do with a case (read from mc_svm_fit.hip, restated here so that the CPU file can check the table):
  * k6_svm_fit: one workgroup of BT = 1024 lanes per solve; lane tid owns the rows t = tid + 1024 r; a block argmax (a lane's rows
    in rising t with a strict `>`, a butterfly over the wave and the 16 waves in order, equal values to the LOWER index) picks i and
    then j; every solve starts with ALL its +1 rows tied at -y G = 1, so the first i is row 0 in every case here, with rivals in the
    same wave, in other waves and (from 1025 rows of the first class on) in the lane's next stride;
  * k6_svm_val: a grid of ceil(max_va / 256) x jobs blocks of 256, a lane per held-out row, jobs shorter than max_va idle;
  * k6_svm_sigmoid: one workgroup of ST = 1024 lanes, every sum in the fixed order svm_fit_oracle.sigmoid_train(order='device') restates.

SOLVE cases compare alpha ITSELF at a capped iterate (status 1, n_iter = cap) or at convergence, not only the KKT gap and the dual
objective, which cannot see which of two equal rows was taken or a wrong row whose alpha stays 0.  The acceptance is
    |alpha_dev - alpha_oracle|.max() <= 16 alpha_wobble + 1e-12 C
where alpha_wobble is the largest change of any alpha when every kernel value of the oracle is multiplied by 1 +- 2^-52 (two seeds;
an exp one ulp off; equal arguments keep equal values, so constructed ties stay ties).  The CPU file requires that the wobble leaves
the trace and n_iter as they are, and that every selection gap is exactly 0 (a constructed tie) or at least GAP_MIN.

The measured values: WOBBLE below (tests/test_svm_fit_cases.py recomputes them): at most 2e-14 at C = 1, 9.5e-11 at C = 1000.

Branches, exits and mutants held (the CPU file computes the table and holds it to HELD / CATCHES): all eight clipping branches, tau in
the selection and in the update (`contradict`: the same point under both labels), rho by mean and by midpoint (`all_at_C`: every
alpha at the bound, without a single duplicate), the exits by max_iter and by convergence.  UNREACHED, by any input: the exit
`i < 0` (I_up empty) needs every +1 row at C and every -1 row at 0, and the pair updates keep sum y alpha = 0, which would then
read C n_+ = 0.  UNCAUGHT: tau_ignored (NOT_MOVED says why).

What a case may NOT contain (decisive(), held by the CPU file for every solve, plain and wobbled): a selection decided by less than
GAP_MIN that is not a constructed tie.  Two rows just updated as a pair have equal values mathematically and values a rounding apart
in floating point; where they are the two best candidates of the next selection, libsvm's own choice is an accident of its exp.
Such solves (a lone +1 row after its second step; about half the draws of the 63- to 65-row problems within 40 steps) are capped
earlier or drawn again.

SIGMOID cases: n in {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}, one class only (the gradient is below eps at entry: the starting
point comes back bit for bit), all-zero decision values, separable and anti-correlated values, and |dec| up to 1e3, where the Newton
step overshoots: one accepted halving (`backtrack_two_points`), and searches that halve 34 times and leave by min_step.  Separable
values of ordinary size do NOT backtrack (0 halvings in every draw); the backtracking inputs were found by a search of 13440 inputs
(tests/test_svm_fit_cases.py::SIGMOID_EXITS), of which those were kept whose trace and (A, B) do not hang on the order of addition:
at |dec| = 1e3 most do (the search then compares sums that differ in the last bits), and none at n >= 1025 passed.  The exit after 100
iterations is unreached.  A constant decision value other than 0 does not determine (A, B) at all: CONSTANT_DEC."""
import functools

import numpy as np

from tests import svm_fit_oracle as so

N_VAL = 70
GAP_MIN = 1e-8
WOBBLE_SEEDS = (1, 2)
TOL_AB = 1e-12             # the project's acceptance for probA and probB (tests/test_gpu_svm_fit.py)
CONVERGE = 100000          # max_iter of the cases that run to convergence


def _solve(name, edge, l, d=3, C=1.0, max_iter=40, kind='normal', seed=1, first=0, **expect):
    return dict(name=name, edge=edge, l=l, d=d, C=C, max_iter=max_iter, kind=kind, seed=seed, first=first, expect=expect)


def _table():
    t = []
    # ---- training sizes on the lane, wave and block boundaries ----
    for l in (2, 63, 64, 65, 1023, 1024, 1025, 2049):
        t.append(_solve('rows_%d' % l, 'rows', l, max_iter=1 if l == 2 else 40))
    # ---- one row of one class against l - 1 of the other, the lone row as +1 (first) and as -1 (last) ----
    # (lone as +1: after two steps the only candidates for i are the two -1 rows just updated as a pair, whose values are EQUAL
    # mathematically and a rounding apart in floating point -- libsvm's choice there is an accident of its exp; the cap stops before)
    for l in (65, 1025):
        t.append(_solve('lone_first_%d' % l, 'lone', l, kind='lone', first=0, max_iter=2))
        t.append(_solve('lone_last_%d' % l, 'lone', l, kind='lone', first=1, max_iter=30))
    # ---- widths ----
    for d in (1, 64):
        t.append(_solve('width_%d' % d, 'width', 130, d=d))
    # ---- exact ties: every row has a bit-equal twin m rows on -- in its wave, in the next wave, in its lane's next stride ----
    t.append(_solve('twins_one_wave', 'ties', 64, kind='twins', max_iter=CONVERGE, twin_distance=32))
    t.append(_solve('twins_two_waves', 'ties', 128, kind='twins', max_iter=CONVERGE, twin_distance=64))
    t.append(_solve('twins_two_strides', 'ties', 2048, kind='twins', max_iter=60, twin_distance=1024))
    # ---- the same point under both labels: quad <= 0 -> TAU in the selection and in the update ----
    t.append(_solve('contradict', 'tau', 64, kind='contradict', max_iter=CONVERGE))
    # ---- both ends of C ----
    t.append(_solve('C_small', 'C', 130, C=0.01, max_iter=300))
    t.append(_solve('C_large', 'C', 130, C=1000.0, max_iter=300))
    t.append(_solve('all_at_C', 'rho', 64, C=0.01, kind='balanced', max_iter=CONVERGE))
    # ---- iterates ----
    for cap in (1, 2, 20):
        t.append(_solve('iterate_%d' % cap, 'iterate', 130, max_iter=cap))
    t.append(_solve('converges', 'iterate', 24, kind='easy', max_iter=CONVERGE))
    return {c['name']: c for c in t}


CASES = _table()
# data seeds other than 1: picked so that every selection gap of the oracle's solve is exactly 0 or at least GAP_MIN, with and without the
# wobble, and so that the table as a whole takes all eight clipping branches (conditions on the inputs: tests/test_svm_fit_cases.py
# holds them for every case)
DATA_SEEDS = {'rows_63': 5, 'rows_64': 2, 'rows_65': 6, 'lone_last_65': 13, 'lone_last_1025': 6, 'twins_one_wave': 3, 'contradict': 3,
              'C_large': 11, 'converges': 5}
for _name, _seed in DATA_SEEDS.items():
    CASES[_name]['seed'] = _seed
# alpha_wobble per job as measured where the table was made, for the record; the tolerance uses the value measured where the test runs
# (alpha_tolerance), which tests/test_svm_fit_cases.py holds within a factor of 4 of this one: 0 where the capped solve only ever
# clips to the bounds 0 and C, which no kernel value enters
WOBBLE = {'C_large': (9.5e-11,),
 'C_small': (0.0,),
 'all_at_C': (0.0,),
 'contradict': (1.3e-14,),
 'converges': (5.2e-16,),
 'iterate_1': (0.0,),
 'iterate_2': (0.0,),
 'iterate_20': (0.0,),
 'lone_first_1025': (4e-15,),
 'lone_first_65': (7e-16,),
 'lone_last_1025': (4.9e-15,),
 'lone_last_65': (1.2e-14,),
 'multi_job': (0.0, 0.0, 5.7e-15),
 'rows_1023': (0.0,),
 'rows_1024': (0.0,),
 'rows_1025': (0.0,),
 'rows_2': (0.0,),
 'rows_2049': (0.0,),
 'rows_63': (1.3e-15,),
 'rows_64': (5.5e-15,),
 'rows_65': (1.1e-14,),
 'twins_one_wave': (1.5e-14,),
 'twins_two_strides': (0.0,),
 'twins_two_waves': (2e-14,),
 'width_1': (0.0,),
 'width_64': (0.0,)}

# per case the mutants (svm_fit_oracle.SMO_MUTANTS) that touch a branch it takes and move alpha -- rho for rho_midpoint_as_mean -- by
# 1000 times the GPU tolerance and more; tests/test_svm_fit_cases.py recomputes the table.  Every mutant but tau_ignored is caught.
CATCHES = {'C_large': ('ties_to_highest_index', 'skip_diff_pos_aj_below_0', 'skip_diff_pos_ai_above_C', 'skip_diff_neg_aj_above_C',
             'skip_sum_small_aj_below_0', 'skip_sum_small_ai_below_0'),
 'C_small': ('skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'all_at_C': ('skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'contradict': ('ties_to_highest_index', 'skip_diff_pos_ai_above_C', 'skip_diff_neg_aj_above_C', 'skip_sum_small_ai_below_0'),
 'converges': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'skip_sum_small_aj_below_0', 'skip_sum_small_ai_below_0'),
 'iterate_1': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'iterate_2': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'iterate_20': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'skip_sum_small_aj_below_0'),
 'lone_first_1025': ('skip_diff_neg_aj_above_C',),
 'lone_first_65': ('skip_diff_neg_aj_above_C',),
 'lone_last_1025': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'skip_sum_small_aj_below_0'),
 'lone_last_65': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'skip_sum_small_aj_below_0'),
 'rows_1023': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'rows_1024': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'rows_1025': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'rows_2': ('skip_diff_neg_aj_above_C',),
 'rows_2049': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'rows_63': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'skip_sum_big_ai_above_C', 'skip_sum_big_aj_above_C'),
 'rows_64': ('ties_to_highest_index', 'skip_diff_pos_aj_below_0', 'skip_diff_neg_aj_above_C', 'skip_sum_small_ai_below_0'),
 'rows_65': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'skip_sum_big_ai_above_C', 'skip_sum_small_aj_below_0',
             'skip_sum_big_aj_above_C', 'skip_sum_small_ai_below_0'),
 'twins_one_wave': ('ties_to_highest_index', 'skip_diff_pos_aj_below_0', 'skip_diff_pos_ai_above_C', 'skip_diff_neg_aj_above_C'),
 'twins_two_strides': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'twins_two_waves': ('ties_to_highest_index', 'skip_diff_neg_ai_below_0', 'skip_diff_neg_aj_above_C', 'skip_sum_big_ai_above_C',
                     'skip_sum_small_aj_below_0', 'skip_sum_big_aj_above_C'),
 'width_1': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean'),
 'width_64': ('ties_to_highest_index', 'skip_diff_neg_aj_above_C', 'rho_midpoint_as_mean')}

# mutants that touch a case's branch and move NOTHING, with the reason
NOT_MOVED = {
    ('rows_2', 'ties_to_highest_index'): 'one +1 row: no rival',
    ('rows_2', 'rho_midpoint_as_mean'): 'two rows: the mean of both is the midpoint',
    ('lone_first_65', 'ties_to_highest_index'): 'one +1 row, and two steps without a tie',
    ('lone_first_1025', 'ties_to_highest_index'): 'one +1 row, and two steps without a tie',
    ('C_small', 'ties_to_highest_index'): 'every alpha ends at C whichever row goes first',
    ('all_at_C', 'ties_to_highest_index'): 'every alpha ends at C whichever row goes first',
    ('contradict', 'tau_ignored'): 'quad is exactly 0, never negative (K <= 1): IEEE division gives an infinite step, which the '
                                   'clipping cuts to the same bounds as the step over TAU -- UNCAUGHT by any case, by nature',
}

MULTI_L, MULTI_VA, MULTI_FIRST = (2, 1025, 65), (257, 0, 255), (1, 0, 1)
MULTI = dict(name='multi_job', edge='jobs', d=3, C=1.0, max_iter=40, seed=9, expect={})


def _rows(rng, n, d, margin=0.0):
    X = rng.normal(size=(n, d)) * np.linspace(0.5, 2.0, d)
    z = X[:, 0] - 0.5 * X[:, -1] + 0.4 * rng.normal(size=n)
    y = (z > 0).astype(np.uint8)
    if margin:
        X[:, 0] += np.where(y == 1, margin, -margin)
    return X, y


def problem(case):
    """-> X, y, [(training rows in solve order, held-out rows)], [gamma]."""
    l, d, kind = case['l'], case['d'], case['kind']
    rng = np.random.default_rng([case['seed'], l, d])
    X, y = _rows(rng, l + N_VAL, d, margin=3.0 if kind == 'easy' else 0.0)
    rows = np.arange(l)
    if kind == 'lone':                                       # row 0 alone in class `first`
        y[:l] = 1 - case['first']
        y[0] = case['first']
    elif kind == 'twins':                                    # row t + m is row t again
        m = l // 2
        X[m:l], y[m:l] = X[:m], y[:m]
    elif kind == 'contradict':                               # rows 48.. are rows 0..15 again, under the other label
        X[48:64], y[48:64] = X[:16], 1 - y[:16]
    elif kind == 'balanced':
        y[:l] = np.arange(l) % 2
    if len(np.unique(y[:l])) < 2:
        y[0], y[1] = 0, 1
    if kind in ('twins', 'contradict'):
        train = rows                                         # (the twins stay m rows apart: the first row's class is the solve's +1)
    elif kind == 'lone':
        train = so.grouped(rows, y, 0)                       # row 0 first when it is class 0, last when it is class 1
    else:
        train = so.grouped(rows, y, case['first'])
    return np.ascontiguousarray(X), y, [(train, np.arange(l, l + N_VAL))], [so.gamma_of(X[train])]


def multi_problem():
    rng = np.random.default_rng([MULTI['seed'], 99])
    n = sum(MULTI_L) + sum(MULTI_VA)
    X, y = _rows(rng, n, MULTI['d'])
    jobs, at = [], 0
    for l, nv, first in zip(MULTI_L, MULTI_VA, MULTI_FIRST):
        y[at], y[at + 1] = 0, 1
        jobs.append((so.grouped(np.arange(at, at + l), y, first), np.arange(at + l, at + l + nv)))
        at += l + nv
    return np.ascontiguousarray(X), y, jobs, [so.gamma_of(X[tr]) for tr, _ in jobs]


def labels(y, train):
    return np.where(y[train] == y[train[0]], 1.0, -1.0)


def solve(case, X, y, train, gamma, **kw):
    return so.smo(X[train], labels(y, train), gamma, C=case['C'], max_iter=case['max_iter'], **kw)


def problem_of(case):
    return multi_problem() if case is MULTI else problem(case)


def decisive(trace, Xt, ys):
    """Every selection of a solve on the rows Xt with labels ys is decided by GAP_MIN and more, or is a CONSTRUCTED tie: gap exactly
    0 between two rows that are bit-equal with equal labels (twins), or between candidates for i whose G is still the initial -1
    (-y G = 1 exactly: the first selection, and the selections after a pair of bit-equal rows under opposite labels, whose step
    changes no G at all).
    Two rows just updated as a pair have EQUAL values mathematically and values a rounding apart in floating point -- sometimes exactly
    equal: such a tie is an accident of the arithmetic, another exp decides it the other way, and a case must not contain one."""
    for k, (i, ri, j, rj, gmax) in enumerate(trace['picks']):
        for gap, a, b, untouched in ((trace['gap_i'][k], i, ri, gmax == 1.0), (trace['gap_j'][k], j, rj, False)):
            if gap >= GAP_MIN:
                continue
            twins = b >= 0 and ys[a] == ys[b] and (Xt[a] == Xt[b]).all()
            if gap != 0 or not (twins or untouched):
                return False
    return True


def solve_all(case):
    """The oracle's solves of the case's jobs, each with its trace (uncached)."""
    X, y, jobs, gammas = problem_of(case)
    out = []
    for (tr, va), g in zip(jobs, gammas):
        trace = {}
        s = solve(case, X, y, tr, g, trace=trace)
        s['trace'] = trace
        out.append(s)
    return tuple(out)


def wobble_all(case, wants):
    """Per job (alpha_wobble, same): the largest change of any alpha under WOBBLE_SEEDS, and whether every wobbled solve went the way
    the plain one went -- n_iter, status, branches, the same selections tied, every gap decisive, the same support (uncached)."""
    X, y, jobs, gammas = problem_of(case)
    out = []
    for (tr, va), g, want in zip(jobs, gammas, wants):
        worst, same = 0.0, True
        zeros = [[v == 0 for v in want['trace'][k]] for k in ('gap_i', 'gap_j')]
        for seed in WOBBLE_SEEDS:
            trace = {}
            s = solve(case, X, y, tr, g, trace=trace, wobble=seed)
            same = same and s['n_iter'] == want['n_iter'] and s['status'] == want['status'] and \
                trace['branches'] == want['trace']['branches'] and decisive(trace, X[tr], labels(y, tr)) and \
                [[v == 0 for v in trace[k]] for k in ('gap_i', 'gap_j')] == zeros and [(p[0], p[2]) for p in trace['picks']] == [(p[0], p[2]) for p in want['trace']['picks']] and \
                bool(((s['alpha'] > 0) == (want['alpha'] > 0)).all())
            worst = max(worst, float(np.abs(s['alpha'] - want['alpha']).max()))
        out.append((worst, same))
    return tuple(out)


def _case_of(name):
    return MULTI if name == MULTI['name'] else CASES[name]


@functools.lru_cache(maxsize=None)
def _oracle_by_name(name):
    return solve_all(_case_of(name))


def oracle(case):
    """The oracle's solves of the case's jobs with their traces, computed once and shared: do not write into them."""
    return _oracle_by_name(case['name'])


@functools.lru_cache(maxsize=None)
def _wobble_by_name(name):
    return wobble_all(_case_of(name), _oracle_by_name(name))


def wobble(case):
    """Per job (alpha_wobble, whether both wobbled solves went the way the plain one went)."""
    return _wobble_by_name(case['name'])


def alpha_tolerance(case, job=0):
    """16 alpha_wobble + 1e-12 C: the wobble is measured on the reference under a one-ulp exp, the factor is for an exp up to a few
    ulps off over a few dozen updates, the floor covers the cases whose wobble is 0."""
    measured = wobble(case)[job][0]
    case['expect'].setdefault('alpha_wobble', {})[job] = measured
    return 16.0 * measured + 1e-12 * case['C']


def val_decision(X, y, train, val, gamma, alpha, rho):
    """k6_svm_val's value from GIVEN alpha and rho: the support vectors in order, the difference form, turned so that > 0 means
    class 0."""
    from tests import svm_oracle
    ys = labels(y, train)
    sv = alpha > 0
    dec = svm_oracle.decision(X[train][sv], (ys * alpha)[sv], gamma, -rho, X[val])
    return dec if y[train[0]] == 0 else -dec


# ------------------------------------------------------------------ the Platt solver
def _sig(name, n, kind='normal', seed=1, scale=1.0, **expect):
    return dict(name=name, n=n, kind=kind, seed=seed, scale=scale, expect=expect)


def _sigmoid_table():
    t = [_sig('n_%d' % n, n) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)]
    t += [_sig('one_class_0', 65, 'one_class_0', exit='gradient_at_entry'), _sig('one_class_1', 1025, 'one_class_1', exit='gradient_at_entry'),
          _sig('zero_dec', 130, 'zero'), _sig('separable', 130, 'separable'), _sig('separable_1025', 1025, 'separable'),
          _sig('anti', 130, 'anti'),
          # ---- |dec| up to 1e3: the Newton step overshoots and the line search backtracks; a search that finds no step ----
          _sig('backtrack_two_points', 65, 'two_points', seed=4, scale=300.0, exit='gradient', halvings=1),
          _sig('backtrack_then_min_step', 65, 'two_points', seed=29, scale=1000.0, exit='min_step', halvings=37),
          _sig('min_step_two_points', 65, 'two_points', seed=10, scale=1000.0, exit='min_step', halvings=34),
          _sig('min_step_normal_130', 130, 'normal', seed=17, scale=300.0, exit='min_step', halvings=34),
          _sig('min_step_anti_130', 130, 'anti', seed=17, scale=300.0, exit='min_step', halvings=34),
          _sig('min_step_noisy_130', 130, 'noisy', seed=24, scale=30.0, exit='min_step', halvings=34),
          _sig('big_dec_130', 130, 'normal', seed=20, scale=1000.0, exit='min_step', halvings=35)]
    return {c['name']: c for c in t}


SIGMOID_CASES = _sigmoid_table()
# A constant decision value other than 0 does not determine (A, B): the Hessian's determinant is sigma (1e-12) times the sum, below the
# rounding of its two products, and the order of addition moves (A, B) by 1e-3 of themselves.  What IS determined is the fitted
# probability p at that value: the solver leaves by |g2| = |sum t - n p| < 1e-5, so two right solvers agree on p within 2e-5 / n.
CONSTANT_DEC = _sig('constant_dec', 130, 'constant', scale=1.0)


def sigmoid_problem(case):
    """-> dec, y (0: libsvm's +1)."""
    n, kind, scale = case['n'], case['kind'], case['scale']
    rng = np.random.default_rng([case['seed'], n, 17])
    y = rng.integers(0, 2, n).astype(np.uint8)
    if n >= 2:
        y[0], y[1] = 0, 1
    lab = np.where(y == 0, 1.0, -1.0)
    base = rng.normal(size=n)
    dec = (1.2 * lab + base) * scale
    if kind == 'one_class_0':
        y[:] = 0
    elif kind == 'one_class_1':
        y[:] = 1
    elif kind == 'constant':
        dec[:] = 0.75 * scale
    elif kind == 'zero':
        dec[:] = 0.0
    elif kind == 'separable':
        dec = lab * (0.5 + np.abs(rng.normal(size=n)))
    elif kind == 'two_points':                               # +scale for one class, -scale for the other
        dec = lab * scale
    elif kind == 'noisy':
        dec = (0.3 * lab + base) * scale
    elif kind == 'anti':
        dec = -dec
    elif kind != 'normal':
        raise ValueError(kind)
    dec = np.clip(dec, -1e3, 1e3)
    return np.ascontiguousarray(dec), y


@functools.lru_cache(maxsize=None)
def _sigmoid_by_name(name):
    dec, y = sigmoid_problem(CONSTANT_DEC if name == CONSTANT_DEC['name'] else SIGMOID_CASES[name])
    trace = {}
    A, B = so.sigmoid_train(dec, np.where(y == 0, 1.0, -1.0), trace=trace)
    return A, B, trace


def sigmoid_oracle(case):
    return _sigmoid_by_name(case['name'])


def fitted(A, B, dec):
    """libsvm's sigmoid_predict: the probability of the +1 class at a decision value."""
    f = dec * A + B
    return float(np.exp(-f) / (1.0 + np.exp(-f)) if f >= 0 else 1.0 / (1.0 + np.exp(f)))
