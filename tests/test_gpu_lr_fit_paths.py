"""The LR fit kernel (k7_lr_fit) on the case table of tests/lr_fit_cases.py: the solver's rarely taken branches (line-search halving
and exhaustion, the 1000-sweep cap, the step clipped at +-10, shrinking and reactivation, w = 0) compared with the oracle at the
same capped ITERATE, and the row loops' lane, wave and block edges.  What each case is for: tests/lr_fit_cases.py; that the table
holds what it says: tests/test_lr_fit_cases.py."""
import numpy as np
import pytest

from tests import lr_fit_cases as LC
from tests import lr_fit_oracle as lo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def hold(X, y, va, got, want):
    wg = np.concatenate([got['coef'], [got['intercept']]])
    ww = want['w']
    assert (got['status'], got['n_iter']) == (want['status'], want['n_iter'])
    err = np.abs(wg - ww).max()
    print('w off by %.3e, bound %.3e' % (err, LC.tolerance(ww)))
    assert err <= LC.tolerance(ww)                                          # (TOL_W max(1, |w|max), at the iterate)
    assert ((wg == 0) == (ww == 0)).all()
    # the held-out rows from the device's OWN w: the decision values to 1e-12, the count exactly
    assert got['n_val'] == len(va) == len(got['val_dec'])
    if len(va):
        assert np.abs(got['val_dec'] - lo.decision(X[va], wg)).max() <= 1e-12
        assert got['val_correct'] == int(((got['val_dec'] > 0).astype(np.int64) == y[va]).sum())
    else:
        assert got['val_correct'] == 0


@pytest.mark.parametrize('name', sorted(LC.CASES))
def test_lr_fit_equals_the_oracle_at_the_same_iterate(dev, name):
    c = LC.CASES[name]
    X, y, jobs = LC.problem(c)
    kw = dict(C=c['C'], max_iter=c['max_iter'])
    [got] = dev.lr_fit(X, y, jobs, [c['lr_seed']], **kw)
    [again] = dev.lr_fit(X, y, jobs, [c['lr_seed']], **kw)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), k
    hold(X, y, jobs[0][1], got, LC.oracle(c)[0])


def test_lr_jobs_of_mixed_sizes_in_one_call(dev):
    c = LC.MULTI
    X, y, jobs = LC.multi_problem()
    got = dev.lr_fit(X, y, jobs, list(c['lr_seeds']), C=c['C'], max_iter=c['max_iter'])
    for (tr, va), fit, want in zip(jobs, got, LC.oracle(c)):
        hold(X, y, va, fit, want)
    alone = [dev.lr_fit(X, y, [j], [s], C=c['C'], max_iter=c['max_iter'])[0] for j, s in zip(jobs, c['lr_seeds'])]
    for a, b in zip(got, alone):                                            # a job's fit does not depend on its neighbours
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_lr_context_still_fits_a_plain_problem_afterwards(dev):
    c = LC.CASES['width_1']
    X, y, jobs = LC.problem(c)
    [got] = dev.lr_fit(X, y, jobs, [c['lr_seed']], C=c['C'], max_iter=c['max_iter'])
    hold(X, y, jobs[0][1], got, LC.oracle(c)[0])
