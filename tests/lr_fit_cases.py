"""Small problems for the LR fit kernel (k7_lr_fit, csrc/mc_simple_fit.hip): PATH cases, one per branch of liblinear's newGLMNET that the
seeded problems of tests/test_gpu_simple_fit.py never take, and SHAPE cases on the lane, wave and block boundaries of the kernel's row
loops.  A case is a seeded generator call plus parameters; the yardstick is tests/lr_fit_oracle.py::solve on the same rows, seed and
parameters (`oracle(case)`, computed once per process).  tests/test_lr_fit_cases.py checks on the CPU that every case takes the branch
it names before its cap, that the order of addition does not decide it and that a kernel wrong in that branch would fail it;
tests/test_gpu_lr_fit_paths.py holds the kernel to the table.

PATH cases fix max_iter to a cap: the first Newton iteration (counted from 1) in which the oracle takes the named branch, plus one
(that iteration itself where the solve would stop of its own accord right after it: the four overflow cases).
The device and the oracle are then compared at the same ITERATE (status 1, n_iter = cap), where a wrong step still shows, not at the
optimum, which many wrong iterations reach as well.  The family is X = N(0, 1) scale, y = (X[:, 0] > 0), optionally with label
noise; the parameters below come from a search of 2400 draws of it (l in {12, 30, 70, 130, 260, 520, 600}, d in {1, 2, 5},
scale = 10^U(-3, 1.5), C = 10^U(0, 5), both rounded to two digits, label noise in {0, 0, 0.05, 0.2}, 30 Newton iterations each):

  branch                                   draws that took it (of 2400)
  |z| < 1e-12 skipped                      1906
  z clipped to +10 / to -10                1275 / 301
  outer shrink / inner shrink+reactivation  520 / 316
  a line-search halving                     148   (all but ONE through an overflow: exp(xTd) exp_wTx = inf, cond = NaN, `cond <= 0`
                                                   false -- liblinear's behaviour, and the kernel's `cond <= 0` goes the same way)
  line search exhausted (20 halvings)       138   (every one with non-finite intermediates, every one but one with the 1000-sweep cap
                                                   in the same or the previous iteration: NO draw exhausts the search with finite
                                                   numbers; separable rows and a large C drive exp_wTx to inf first)
  1000 coordinate-descent sweeps            137
  w stays 0 (n_iter 0)                       12

Two further searches looked for what that one did not find: 800 draws at l in {130, 520, 600}, d in {2, 5}, scale 1 .. 10,
C 30 .. 3000 with 2 .. 10 % label noise (the neighbourhood of the one finite halving) and 3000 draws of the first family at
l in {520, 600, 700, 1025}, 40 and 30 Newton iterations each.

UNREACHED in all 6200 draws, and without a GPU test:
  * the `QP_no_change >= 10` stop and an emptied QP active set (ten Newton iterations in a row without a single |z| >= 1e-12 would
    have met the gradient stop long before);
  * line-search exhaustion with finite intermediates;
  * an accepted halving with finite intermediates at l above 512 (the one finite halving is at l = 12: `halving_finite_l12`; above
    512 the halvings of `halving_l600` and `halvings_3_l600` follow an overflow).  What a finite halving adds is the factor on
    negsum_xTd, a scalar on thread 0, which does not depend on l; the halving of xTd over more than one stride is held by the two.

MUTANTS (lr_fit_oracle.MUTANTS) and the cases that catch them: CATCHES below, which tests/test_lr_fit_cases.py recomputes; a mutant
moves a case when max |w_mutant - w| at the cap is at least 1000 times the GPU tolerance.  Every mutant is caught by a case but
no_recompute_after_exhaust: after an exhausted search tau and D stay as they were, so the next model, its step and its search are
the same again and are exhausted again -- w never moves after the first exhaustion in any draw, and the recomputed exp_wTx is
never read into an accepted step (NOT_MOVED).

SHAPE cases: l in {2, 63, 64, 65, 511, 512, 513, 1025} with n_neg in {1, l - 1} (a lane's, a wave's and the block's last row; the
`t < nneg` split at either end), n_neg = 512 of 1024 and 513 of 1025 (the split on the block edge), d in {1, 63, 64} (n = d + 1 = 65
puts the bias column on the second wave of `tid < n`), and one call with jobs of l = (2, 65, 513, 3) and held-out sizes
(0, 1, 513, 64) (odd offsets into every per-row array).  Shape cases run 6 Newton iterations at C = 1."""
import functools
import warnings

import numpy as np

from tests import lr_fit_oracle as lo

N_VAL = 64
TOL_W = 1e-9               # the project's acceptance (tests/test_gpu_simple_fit.py::assert_lr_matches): |dw| <= TOL_W max(1, |w|max)


def _path(name, edge, seed, l, d, scale, C, noise, cap, **expect):
    return dict(name=name, kind='path', edge=edge, seed=seed, l=l, d=d, scale=scale, C=C, noise=noise, max_iter=cap, lr_seed=77,
                n_neg=None, expect=expect)


def _shape(name, l, n_neg, d, **expect):
    return dict(name=name, kind='shape', edge='shape', seed=3, l=l, d=d, scale=1.0, C=1.0, noise=0.0, max_iter=6, lr_seed=1234567 + l,
                n_neg=n_neg, expect=expect)


def _table():
    t = [
        # ---- line search: one accepted halving (below and above one stride of the block), several in one iteration ----
        _path('halving_finite_l12', 'halving', 431, 12, 5, 2.5, 380.0, 0.05, 18, halvings=1, nonfinite=False),
        _path('halving_l70', 'halving', 445, 70, 1, 31.0, 120.0, 0.0, 13, halvings=1, nonfinite=True),
        _path('halving_l600', 'halving', 578, 600, 1, 4.6, 78.0, 0.0, 13, halvings=1, nonfinite=True),
        _path('halvings_2_l260', 'halvings', 547, 260, 1, 23.0, 4000.0, 0.0, 13, halvings=2, nonfinite=True),
        _path('halvings_3_l600', 'halvings', 1100, 600, 1, 19.0, 22.0, 0.0, 13, halvings=3, nonfinite=True),
        # ---- line search exhausted, exp_wTx recomputed from w; the 1000-sweep cap ----
        _path('exhausted_l70', 'exhausted', 1370, 70, 2, 7.2, 36000.0, 0.0, 14, halvings=20, nonfinite=True),
        _path('exhausted_l12', 'exhausted', 1079, 12, 2, 5.0, 16000.0, 0.0, 16, halvings=20, nonfinite=True),
        # ---- the step clipped to +10 and to -10 ----
        _path('clip_l12', 'clip', 213, 12, 2, 0.0031, 2400.0, 0.05, 2),
        _path('clip_l600', 'clip', 1734, 600, 2, 0.0014, 610.0, 0.0, 2),
        # ---- inner shrinking followed by reactivation; outer shrinking of the bias column ----
        _path('shrink_reactivate_l12', 'inner_shrink', 148, 12, 5, 0.2, 12.0, 0.0, 3),
        _path('shrink_reactivate_l520', 'inner_shrink', 764, 520, 2, 0.0027, 300.0, 0.0, 3),
        _path('shrink_reactivate_l600', 'inner_shrink', 1560, 600, 5, 0.0016, 85.0, 0.0, 4),
        _path('outer_shrink_bias_l260', 'outer_shrink_bias', 109, 260, 2, 0.0098, 1.4, 0.05, 3),
        _path('outer_shrink_bias_l520', 'outer_shrink_bias', 241, 520, 5, 1.7, 1.4, 0.0, 5),
        # ---- C so small that the gradient at w = 0 is inside [-1, 1] everywhere: no Newton iteration ----
        _path('w_zero_l12', 'w_zero', 1621, 12, 2, 0.0016, 3.8, 0.0, 5),
        _path('w_zero_l70', 'w_zero', 385, 70, 2, 0.0024, 35.0, 0.2, 5),
    ]
    for l in (2, 63, 64, 65, 511, 512, 513, 1025):
        for n_neg in sorted({1, l - 1}):
            t.append(_shape('rows_%d_neg_%d' % (l, n_neg), l, n_neg, 3))
    t.append(_shape('rows_1024_neg_512', 1024, 512, 3))
    t.append(_shape('rows_1025_neg_513', 1025, 513, 3))
    for d in (1, 63, 64):
        t.append(_shape('width_%d' % d, 130, 61, d))
    return {c['name']: c for c in t}


CASES = _table()
MULTI_L, MULTI_VA = (2, 65, 513, 3), (0, 1, 513, 64)
MULTI = dict(name='multi_job', kind='multi', edge='jobs', seed=4, d=3, C=1.0, max_iter=6, lr_seeds=(11, 12, 13, 14), expect={})

# which counters of the trace say that a mutant's branch was taken before the cap
TOUCHES = {'no_negsum_halving': ('halvings',), 'no_xTd_halving': ('halvings',), 'no_z_clip': ('z_clip_pos', 'z_clip_neg'),
           'no_reactivation': ('reactivation',), 'no_inner_shrink': ('inner_shrink',), 'no_outer_shrink': ('outer_shrink',),
           'no_recompute_after_exhaust': ('ls_exhausted',), 'inner_eps_not_quartered': ('one_sweep',)}

# per path case the mutants that touch a branch it takes and move w at the cap by 1000 TOL_W max(1, |w|max) and more
CATCHES = {
    'halving_finite_l12': ('no_negsum_halving', 'no_xTd_halving', 'no_reactivation', 'no_inner_shrink', 'no_outer_shrink',
                           'inner_eps_not_quartered'),
    'halving_l70': ('no_xTd_halving', 'inner_eps_not_quartered'),
    'halving_l600': ('no_xTd_halving', 'no_z_clip', 'inner_eps_not_quartered'),
    'halvings_2_l260': ('no_xTd_halving', 'inner_eps_not_quartered'),
    'halvings_3_l600': ('no_xTd_halving', 'inner_eps_not_quartered'),
    'exhausted_l70': ('no_xTd_halving', 'inner_eps_not_quartered'),
    'exhausted_l12': ('no_xTd_halving', 'inner_eps_not_quartered'),
    'clip_l12': ('no_z_clip',),
    'clip_l600': ('no_z_clip',),
    'shrink_reactivate_l12': ('no_reactivation', 'no_inner_shrink', 'inner_eps_not_quartered'),
    'shrink_reactivate_l520': ('no_z_clip', 'no_reactivation', 'no_inner_shrink', 'inner_eps_not_quartered'),
    'shrink_reactivate_l600': ('no_z_clip', 'no_reactivation', 'no_inner_shrink', 'no_outer_shrink', 'inner_eps_not_quartered'),
    'outer_shrink_bias_l260': ('no_z_clip', 'no_outer_shrink', 'inner_eps_not_quartered'),
    'outer_shrink_bias_l520': ('no_outer_shrink', 'inner_eps_not_quartered'),
    'w_zero_l12': (),                            # (no Newton iteration: no mutant touches it; held for status, n_iter and w = 0)
    'w_zero_l70': (),
}

# mutants that touch a case's branch and move NOTHING at its cap, with the reason
_NAN_FIRST = 'the first cond is NaN (overflow) and the halved step passes by a wide margin: the factor on negsum_xTd decides nothing'
_FROZEN = 'w does not move in or after an exhausted search'
NOT_MOVED = {
    ('halving_l70', 'no_negsum_halving'): _NAN_FIRST, ('halving_l600', 'no_negsum_halving'): _NAN_FIRST,
    ('halvings_2_l260', 'no_negsum_halving'): _NAN_FIRST, ('halvings_3_l600', 'no_negsum_halving'): _NAN_FIRST,
    ('exhausted_l70', 'no_negsum_halving'): _NAN_FIRST, ('exhausted_l12', 'no_negsum_halving'): _NAN_FIRST,
    ('exhausted_l70', 'no_z_clip'): 'the clipped steps belong to the exhausted iterations: ' + _FROZEN,
    ('exhausted_l70', 'no_recompute_after_exhaust'): _FROZEN + ' -- UNCAUGHT by any case',
    ('exhausted_l12', 'no_recompute_after_exhaust'): _FROZEN + ' -- UNCAUGHT by any case',
    ('clip_l600', 'inner_eps_not_quartered'): 'the one-sweep iteration is the last before the cap',
}


def problem(case):
    """-> X [l + N_VAL, d], y, jobs [(training rows, held-out rows)]."""
    l, d = case['l'], case['d']
    rng = np.random.default_rng([case['seed'], l, d])
    n = l + N_VAL
    if case['kind'] == 'path':
        X = rng.normal(size=(n, d)) * case['scale']
        y = X[:, 0] > 0
        if case['noise'] > 0:
            y = y ^ (rng.random(n) < case['noise'])
        y = y.astype(np.uint8)
        if len(np.unique(y[:l])) < 2:
            y[0], y[1] = 0, 1
    else:                                        # exactly n_neg rows of class 0 among the first l, scattered
        y = np.ones(n, dtype=np.uint8)
        y[rng.permutation(l)[:case['n_neg']]] = 0
        y[l:] = rng.integers(0, 2, N_VAL)
        X = rng.normal(size=(n, d)) * np.linspace(0.5, 3.0, d)
        X[:, 0] += np.where(y == 1, 0.5, -0.5)
    return np.ascontiguousarray(X), y, [(np.arange(l), np.arange(l, n))]


def multi_problem():
    rng = np.random.default_rng([MULTI['seed'], 99])
    n = sum(MULTI_L) + sum(MULTI_VA)
    y = rng.integers(0, 2, n).astype(np.uint8)
    jobs, at = [], 0
    for l, nv in zip(MULTI_L, MULTI_VA):
        y[at], y[at + 1] = 0, 1                  # both classes in every job
        jobs.append((at + rng.permutation(l), np.arange(at + l, at + l + nv)))
        at += l + nv
    X = rng.normal(size=(n, MULTI['d'])) * np.linspace(0.5, 3.0, MULTI['d'])
    X[:, 0] += np.where(y == 1, 0.5, -0.5)
    return np.ascontiguousarray(X), y, jobs


def solve(case, **kw):
    """The oracle on the case's (first) job with the case's parameters; keyword arguments (trace, order, mutate) go to lo.solve."""
    X, y, [(tr, va)] = problem(case)
    with warnings.catch_warnings(), np.errstate(all='ignore'):     # (the overflow cases run through inf and NaN, as liblinear does)
        warnings.simplefilter('ignore')
        return lo.solve_job(X, y, tr, va, case['lr_seed'], C=case['C'], max_iter=case['max_iter'], **kw)


@functools.lru_cache(maxsize=None)
def _oracle_by_name(name):
    if name == MULTI['name']:
        X, y, jobs = multi_problem()
        return tuple(lo.solve_job(X, y, tr, va, s, C=MULTI['C'], max_iter=MULTI['max_iter']) for (tr, va), s in zip(jobs, MULTI['lr_seeds']))
    trace = {}
    out = solve(CASES[name], trace=trace)
    for it in trace['iters'][:-1]:               # (a one-sweep iteration quarters inner_eps for the iterations after it)
        it['one_sweep'] = int(it['sweeps'] == 1)
    trace['total']['one_sweep'] = sum(it['one_sweep'] for it in trace['iters'])
    out['trace'] = trace
    return (out,)


def oracle(case):
    """The oracle's fits of the case's jobs (with their trace, for the single-job cases), computed once and shared: do not write into
    them."""
    return _oracle_by_name(case['name'])


def tolerance(w):
    return TOL_W * max(1.0, float(np.abs(w).max()))
