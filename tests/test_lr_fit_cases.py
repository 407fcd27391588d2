"""The case table of tests/lr_fit_cases.py against the oracle alone (no GPU): every path case takes the branch it names before its cap,
the kernel's order of addition neither turns it nor moves w by a tenth of the GPU tolerance, and the mutants of lr_fit_oracle that
touch its branch move w by a thousand tolerances; the shape cases put their rows where they say.  These are conditions on the inputs
(the draws are picked to keep them), not measurements of the device."""
import numpy as np
import pytest

from tests import lr_fit_cases as LC
from tests import lr_fit_oracle as lo

PATHS = sorted(n for n, c in LC.CASES.items() if c['kind'] == 'path')
SHAPES = sorted(n for n, c in LC.CASES.items() if c['kind'] == 'shape')


def first_iteration(trace, key):
    """The first Newton iteration (from 1) whose counter `key` is not 0, or None."""
    for k, it in enumerate(trace['iters']):
        if it[key]:
            return k + 1
    return None


def plain(iters):
    return [{k: v for k, v in it.items() if k != 'one_sweep' and v} for it in iters]


def test_the_table_holds_what_the_gaps_ask_for():
    shapes = {(c['l'], c['n_neg']) for c in LC.CASES.values() if c['kind'] == 'shape' and c['d'] == 3}
    for l in (2, 63, 64, 65, 511, 512, 513, 1025):
        assert {(l, 1), (l, l - 1)} <= shapes
    assert {(1024, 512), (1025, 513)} <= shapes
    assert {c['d'] for c in LC.CASES.values() if c['name'].startswith('width_')} == {1, 63, 64}
    assert (LC.MULTI_L, LC.MULTI_VA) == ((2, 65, 513, 3), (0, 1, 513, 64))
    edges = {c['edge'] for c in LC.CASES.values()}
    assert {'halving', 'halvings', 'exhausted', 'clip', 'inner_shrink', 'outer_shrink_bias', 'w_zero', 'shape'} <= edges
    halvings = [LC.CASES[n] for n in PATHS if LC.CASES[n]['edge'] == 'halving']
    assert min(c['l'] for c in halvings) < 512 < max(c['l'] for c in halvings)
    assert all(c['l'] <= 2100 for c in LC.CASES.values())


@pytest.mark.parametrize('name', PATHS)
def test_path_case_takes_its_branch_before_the_cap(name):
    c = LC.CASES[name]
    [want] = LC.oracle(c)
    trace, tot, e = want['trace'], want['trace']['total'], c['expect']
    if c['edge'] == 'w_zero':
        assert (want['n_iter'], want['status']) == (0, 0) and (want['w'] == 0).all() and tot['gnorm_stop'] == 1
        return
    assert (want['status'], want['n_iter']) == (1, c['max_iter'])          # compared at the iterate, not at an optimum
    assert np.isfinite(want['w']).all() and (want['w'] != 0).any()
    key = {'halving': 'halvings', 'halvings': 'halvings', 'exhausted': 'ls_exhausted', 'clip': 'z_clip_neg', 'inner_shrink': 'inner_shrink',
           'outer_shrink_bias': 'outer_shrink_bias'}[c['edge']]
    at = first_iteration(trace, key)
    overflow = e.get('nonfinite') and c['edge'] in ('halving', 'halvings')
    assert at is not None and c['max_iter'] == at + (0 if overflow else 1), (at, c['max_iter'])
    if overflow:                                                             # (the solve would stop of itself right after)
        longer = LC.solve(dict(c, max_iter=c['max_iter'] + 1))
        assert (longer['status'], longer['n_iter']) == (0, c['max_iter'])
    if c['edge'] in ('halving', 'halvings'):
        assert trace['iters'][at - 1]['halvings'] == e['halvings'] and tot['ls_exhausted'] == 0
        assert bool(tot['nonfinite']) == e['nonfinite']
        assert (e['halvings'] >= 2) == (c['edge'] == 'halvings')
    if c['edge'] == 'exhausted':
        assert trace['iters'][at - 1]['halvings'] == lo.MAX_LINESEARCH and tot['inner_cap'] >= 1 and tot['nonfinite'] >= 1
        assert first_iteration(trace, 'inner_cap') <= at
    if c['edge'] == 'clip':
        assert tot['z_clip_pos'] >= 1 and tot['z_clip_neg'] >= 1 and np.abs(want['w']).max() >= 10.0
    if c['edge'] == 'inner_shrink':
        assert trace['iters'][at - 1]['reactivation'] >= 1                   # shrunk, then reactivated in the same iteration
    if c['edge'] == 'outer_shrink_bias':
        assert tot['outer_shrink_bias'] >= 1 and (want['w'] == 0).any()      # (the bias column is the last: n - 1)


@pytest.mark.parametrize('name', PATHS + SHAPES)
def test_order_of_addition_does_not_decide_the_case(name):
    c = LC.CASES[name]
    [want] = LC.oracle(c)
    td = {}
    dev = LC.solve(c, order='device', trace=td)
    assert (dev['n_iter'], dev['status']) == (want['n_iter'], want['status'])
    assert plain(td['iters']) == plain(want['trace']['iters'])
    assert np.abs(dev['w'] - want['w']).max() <= 0.1 * LC.tolerance(want['w'])
    assert ((dev['w'] == 0) == (want['w'] == 0)).all()


@pytest.mark.parametrize('name', PATHS)
def test_mutants_that_touch_the_case_move_w(name):
    c = LC.CASES[name]
    [want] = LC.oracle(c)
    tot = want['trace']['total']
    tol = LC.tolerance(want['w'])
    caught = []
    for m in lo.MUTANTS:
        if not any(tot[k] for k in LC.TOUCHES[m]):
            continue
        moved = np.abs(LC.solve(c, mutate=m)['w'] - want['w']).max() / tol
        if (name, m) in LC.NOT_MOVED:
            assert moved == 0
        else:
            assert moved >= 1000, (m, moved)
            caught.append(m)
    assert tuple(caught) == LC.CATCHES[name]
    assert caught or c['edge'] == 'w_zero'


def test_every_mutant_is_caught_or_listed():
    caught = {m for v in LC.CATCHES.values() for m in v}
    assert caught == set(lo.MUTANTS) - {'no_recompute_after_exhaust'}
    assert any(m == 'no_recompute_after_exhaust' for _, m in LC.NOT_MOVED)
    # each path's own mutant is caught by a case of that path
    for edge, m in (('halving', 'no_xTd_halving'), ('halving', 'no_negsum_halving'), ('halvings', 'no_xTd_halving'), ('clip', 'no_z_clip'),
                    ('inner_shrink', 'no_inner_shrink'), ('inner_shrink', 'no_reactivation'), ('outer_shrink_bias', 'no_outer_shrink')):
        assert any(m in LC.CATCHES[n] for n in PATHS if LC.CASES[n]['edge'] == edge), (edge, m)


def test_the_default_suite_never_takes_these_branches():
    """The gap: on the problems of tests/test_gpu_simple_fit.py that a CPU can afford here, no halving, no clip to -10 ... at all."""
    from tests.helpers import fit_data
    seen = {}
    for n, d, rounding in ((5, 1, None), (40, 4, 0), (600, 9, 1)):
        X, y = fit_data(n, d, n + d, rounding)
        if n == 5:
            y = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
        trace = {}
        lo.solve_job(X, y, np.arange(n), np.zeros(0, np.int64), 1234567, trace=trace)
        for k, v in trace['total'].items():
            seen[k] = seen.get(k, 0) + v
    assert not any(seen.get(k) for k in ('halvings', 'ls_exhausted', 'inner_cap', 'z_clip_pos', 'z_clip_neg', 'nonfinite', 'qp_no_change_stop'))


@pytest.mark.parametrize('name', SHAPES)
def test_shape_case_puts_its_rows_where_it_says(name):
    c = LC.CASES[name]
    X, y, [(tr, va)] = LC.problem(c)
    assert X.shape == (c['l'] + LC.N_VAL, c['d']) and int((y[tr] == 0).sum()) == c['n_neg'] and len(tr) == c['l']
    if 2 < c['n_neg'] < c['l'] - 2:
        assert (np.diff(y[tr].astype(int)) != 0).sum() > 2                   # the classes come scattered: the grouping is tested
    [want] = LC.oracle(c)
    assert want['n_iter'] >= 1 and np.isfinite(want['w']).all() and (want['w'] != 0).any()
    assert np.abs(want['val_dec']).min() > 0


def test_multi_job_call():
    X, y, jobs = LC.multi_problem()
    assert [len(tr) for tr, _ in jobs] == list(LC.MULTI_L) and [len(va) for _, va in jobs] == list(LC.MULTI_VA)
    assert np.cumsum(LC.MULTI_L)[:-1].tolist() == [2, 67, 580] and np.cumsum(LC.MULTI_VA)[:-1].tolist() == [0, 1, 514]
    fits = LC.oracle(LC.MULTI)
    assert len({f['n_iter'] for f in fits}) >= 2                             # the jobs leave the Newton loop at different times
    for (tr, va), f in zip(jobs, fits):
        assert set(y[tr].tolist()) == {0, 1} and np.isfinite(f['w']).all()
