"""The SVM fit kernels (k6_svm_fit, k6_svm_val, k6_svm_sigmoid) on the case tables of tests/svm_fit_cases.py: alpha ITSELF against the
oracle's at the same iterate, the support set, rho, status and n_iter; k6_svm_val apart from the solve, on the device's own alpha
and rho; the Platt solver at every size, degenerate input and exit.  What each case is for and where the bounds come from:
tests/svm_fit_cases.py; that the tables hold what they say: tests/test_svm_fit_cases.py."""
import numpy as np
import pytest

from tests import svm_fit_cases as SC
from tests import svm_fit_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def hold_solve(c, X, y, tr, va, gamma, got, want, tol):
    ys = SC.labels(y, tr)
    assert (got['status'], got['n_iter']) == (want['status'], want['n_iter'])
    err = np.abs(got['alpha'] - want['alpha']).max()
    print('alpha off by %.3e, bound %.3e' % (err, tol))
    assert err <= tol
    assert ((got['alpha'] > 0) == (want['alpha'] > 0)).all()                # the support set, exactly
    assert ((got['alpha'] >= c['C']) == (want['alpha'] >= c['C'])).all()
    G = so.gradient(X[tr], ys, want['alpha'], gamma)
    assert abs(got['rho'] - want['rho']) <= tol * max(1.0, np.abs(ys * G).max())
    # the existing checks: the KKT gap of a converged solve, the dual objective
    if want['status'] == 0:
        assert so.kkt_violation(X[tr], ys, got['alpha'], gamma, C=c['C']) <= 1e-3
    sg, sw = got['alpha'] > 0, want['alpha'] > 0
    og = so.dual_objective(X[tr][sg], (ys * got['alpha'])[sg], gamma)
    ow = so.dual_objective(X[tr][sw], (ys * want['alpha'])[sw], gamma)
    assert abs(og - ow) <= 1e-6 * abs(ow)
    hold_val(X, y, tr, va, gamma, got)


def hold_val(X, y, tr, va, gamma, got):
    """k6_svm_val on the device's OWN alpha and rho: the decision values to 1e-12 (k3_svm's tolerance), the count exactly."""
    assert got['n_val'] == len(va) == len(got['val_dec'])
    if not len(va):
        assert got['val_correct'] == 0
        return
    dec = SC.val_decision(X, y, tr, va, gamma, got['alpha'], got['rho'])
    assert np.abs(got['val_dec'] - dec).max() <= 1e-12
    assert got['val_correct'] == int((np.where(got['val_dec'] > 0, 0, 1) == y[va]).sum())


@pytest.mark.parametrize('name', sorted(SC.CASES))
def test_svm_solve_equals_the_oracle_at_the_same_iterate(dev, name):
    c = SC.CASES[name]
    X, y, [(tr, va)], [gamma] = SC.problem(c)
    [got] = dev.svm_fit(X, y, [(tr, va)], [gamma], C=c['C'], max_iter=c['max_iter'])
    [again] = dev.svm_fit(X, y, [(tr, va)], [gamma], C=c['C'], max_iter=c['max_iter'])
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), k
    hold_solve(c, X, y, tr, va, gamma, got, SC.oracle(c)[0], SC.alpha_tolerance(c))


def test_svm_jobs_of_mixed_sizes_and_orientations_in_one_call(dev):
    c = SC.MULTI
    X, y, jobs, gammas = SC.multi_problem()
    got = dev.svm_fit(X, y, jobs, gammas, C=c['C'], max_iter=c['max_iter'])
    for k, ((tr, va), g, fit, want) in enumerate(zip(jobs, gammas, got, SC.oracle(c))):
        hold_solve(c, X, y, tr, va, g, fit, want, SC.alpha_tolerance(c, k))
    assert got[1]['n_val'] == 0 and got[1]['val_correct'] == 0              # no held-out rows: 0
    alone = [dev.svm_fit(X, y, [j], [g], C=c['C'], max_iter=c['max_iter'])[0] for j, g in zip(jobs, gammas)]
    for a, b in zip(got, alone):                                            # a job's solve does not depend on its neighbours
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize('name', sorted(SC.SIGMOID_CASES))
def test_sigmoid_equals_the_oracle(dev, name):
    c = SC.SIGMOID_CASES[name]
    dec, y = SC.sigmoid_problem(c)
    A, B, trace = SC.sigmoid_oracle(c)
    dA, dB = dev.svm_sigmoid_train(dec, y)
    assert (dA, dB) == dev.svm_sigmoid_train(dec, y)
    print('A %.17g (device %.17g), B %.17g (device %.17g), exit %s' % (A, dA, B, dB, trace['exit']))
    if trace['exit'] == 'gradient_at_entry':                                # the starting point, bit for bit
        assert (dA, dB) == (A, B)
    tol = SC.TOL_AB * max(1.0, abs(A), abs(B))
    assert abs(dA - A) <= tol and abs(dB - B) <= tol


def test_sigmoid_of_a_constant_decision_value_fits_the_same_probability(dev):
    """(A, B) are not determined there (tests/svm_fit_cases.py::CONSTANT_DEC); the fitted probability is, within 2e-5 / n."""
    dec, y = SC.sigmoid_problem(SC.CONSTANT_DEC)
    A, B, _ = SC.sigmoid_oracle(SC.CONSTANT_DEC)
    dA, dB = dev.svm_sigmoid_train(dec, y)
    assert np.isfinite([dA, dB]).all()
    assert abs(SC.fitted(dA, dB, dec[0]) - SC.fitted(A, B, dec[0])) <= 2e-5 / len(dec)


def test_svm_context_still_solves_a_plain_problem_afterwards(dev):
    c = SC.CASES['converges']
    X, y, [(tr, va)], [gamma] = SC.problem(c)
    [got] = dev.svm_fit(X, y, [(tr, va)], [gamma])
    hold_solve(c, X, y, tr, va, gamma, got, SC.oracle(c)[0], SC.alpha_tolerance(c))
    dec, yy = SC.sigmoid_problem(SC.SIGMOID_CASES['n_65'])
    A, B, _ = SC.sigmoid_oracle(SC.SIGMOID_CASES['n_65'])
    dA, dB = dev.svm_sigmoid_train(dec, yy)
    assert abs(dA - A) <= SC.TOL_AB * max(1.0, abs(A), abs(B)) and abs(dB - B) <= SC.TOL_AB * max(1.0, abs(A), abs(B))
