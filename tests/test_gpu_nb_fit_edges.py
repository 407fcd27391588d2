"""The NBC fit kernel (k7_nb_fit) on the case table of tests/nb_fit_cases.py: theta, var and epsilon held element by element to the exact
(rational) fit within the bound derived there from the kernel's order of addition; counts exact; ties to class 0.  What each case is
for, and why the bound is what it is: tests/nb_fit_cases.py; that the table holds what it says: tests/test_nb_fit_cases.py."""
import numpy as np
import pytest

from tests import nb_fit_cases as NC
from tests import nb_fit_oracle as no

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def hold(X, y, jobs, got, exact, tie=False):
    assert len(got) == len(jobs)
    for (tr, va), fit, ex in zip(jobs, got, exact):
        bad, worst = NC.check_fit(fit, ex)
        print('largest used fraction of a bound: %.3f' % worst)
        assert not bad, bad
        assert fit['n_val'] == len(va)
        if tie:                                                          # equal joint log-likelihoods: class 0
            assert fit['val_correct'] == int((y[va] == 0).sum())
        else:                                                            # (no held-out row lies in the band: the CPU file)
            assert fit['val_correct'] == no.fit_job(X, y, tr, va)['val_correct']


@pytest.mark.parametrize('name', sorted(NC.CASES))
def test_nb_fit_meets_the_derived_bound(dev, name):
    c = NC.CASES[name]
    X, y, jobs = NC.problem(c)
    got = dev.nb_fit(X, y, jobs, var_smoothing=NC.VAR_SMOOTHING)
    again = dev.nb_fit(X, y, jobs, var_smoothing=NC.VAR_SMOOTHING)
    for a, b in zip(got, again):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    hold(X, y, jobs, got, NC.exact(c), tie=name == 'tie')


def test_nb_jobs_of_mixed_sizes_in_one_call(dev):
    X, y, jobs = NC.multi_problem()
    got = dev.nb_fit(X, y, jobs, var_smoothing=NC.VAR_SMOOTHING)
    hold(X, y, jobs, got, NC.exact(NC.MULTI))
    assert got[0]['val_correct'] == 0 and got[0]['n_val'] == 0            # no held-out rows
    alone = [dev.nb_fit(X, y, [j], var_smoothing=NC.VAR_SMOOTHING)[0] for j in jobs]
    for a, b in zip(got, alone):                                         # a job's fit does not depend on its neighbours
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_nb_context_still_fits_a_plain_problem_afterwards(dev):
    X, y, jobs = NC.problem(NC.CASES['width_7'])
    [fit] = dev.nb_fit(X, y, jobs)
    bad, _ = NC.check_fit(fit, NC.exact(NC.CASES['width_7'])[0])
    assert not bad, bad
