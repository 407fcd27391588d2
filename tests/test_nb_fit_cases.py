"""The case table of tests/nb_fit_cases.py against the exact fit and the NumPy oracle alone (no GPU): every case reaches the edge it
names, the NumPy oracle meets the derived bound against the exact values on every case, and no held-out row but the tie case's lies
inside the band, so that tests/test_gpu_nb_fit_edges.py can ask for EQUAL counts.  These are conditions on the inputs (seeds are
picked to keep them), not measurements of the device."""
from fractions import Fraction

import numpy as np
import pytest

from tests import nb_fit_cases as NC
from tests import nb_fit_oracle as no

ALL = dict(NC.CASES, **{NC.MULTI['name']: NC.MULTI})


def problem_of(c):
    return NC.multi_problem() if c is NC.MULTI else NC.problem(c)


def test_the_table_holds_what_the_gaps_ask_for():
    rows = {(c['l'], c['n0']) for c in NC.CASES.values() if c['edge'] == 'rows'}
    assert {l for l, _ in rows} == {2, 511, 512, 513, 1025}
    for l in (2, 511, 512, 513, 1025):
        assert {(l, 1), (l, l - 1)} <= rows
    assert {(1025, 512), (1025, 513), (513, 512)} <= rows
    assert sorted(c['d'] for c in NC.CASES.values() if c['edge'] == 'width') == [1, 7, 8, 9, 15, 16, 17, 64]
    assert {'const_col', 'const_in_class', 'far_mean', 'var_scales', 'tie'} <= set(NC.CASES)
    assert NC.MULTI_L == (2, 65, 513, 3) and NC.MULTI_VA == (0, 1, 513, 64)
    assert all(c['l'] <= 2100 for c in ALL.values())


@pytest.mark.parametrize('name', sorted(ALL))
def test_case_reaches_its_edge_and_numpy_meets_the_bound(name):
    c = ALL[name]
    X, y, jobs = problem_of(c)
    exs = NC.exact(c)
    if c is NC.MULTI:
        assert [len(tr) for tr, _ in jobs] == list(NC.MULTI_L) and [len(va) for _, va in jobs] == list(NC.MULTI_VA)
        assert np.cumsum([len(tr) for tr, _ in jobs])[:-1].tolist() == [2, 67, 580]          # odd offsets into the grouped rows
        assert np.cumsum([len(va) for _, va in jobs])[:-1].tolist() == [0, 1, 514]
    else:
        assert X.shape == (c['l'] + NC.N_VAL, c['d']) and len(jobs) == 1
    for (tr, va), ex in zip(jobs, exs):
        assert set(y[tr].tolist()) == {0, 1}
        if c is not NC.MULTI:
            assert ex['count'] == [c['n0'], c['l'] - c['n0']]
            assert (np.diff(y[tr].astype(int)) != 0).sum() > 1 or c['l'] <= 3 or 1 in ex['count']    # the classes come scattered
        want = no.fit_job(X, y, tr, va)
        bad, worst = NC.check_fit(want, ex)
        assert not bad, bad
        assert worst <= 0.9, worst                                       # (the margin the docstring speaks of)
        assert ex['E'] > 0
        band = NC.band_rows(want, X, va)
        if name == 'tie':
            jll = no.joint_log_likelihood(want, X[va])
            assert (jll[:, 0] == jll[:, 1]).all() and band == len(va)
            assert want['val_correct'] == int((y[va] == 0).sum()) and 0 < want['val_correct'] < len(va)
        else:
            assert band == 0


@pytest.mark.parametrize('name', sorted(n for n, c in NC.CASES.items() if c['edge'] == 'rows'))
def test_row_cases_put_the_split_where_they_say(name):
    c = NC.CASES[name]
    e = c['expect']
    assert e['n1'] == c['l'] - c['n0'] and e['one_row_class'] == (1 in (c['n0'], e['n1']))
    assert e['strides0'] == -(-c['n0'] // NC.BT) and e['strides1'] == -(-e['n1'] // NC.BT)
    [ex] = NC.exact(c)
    for cls, m in ((0, c['n0']), (1, e['n1'])):
        if m == 1:                                                       # a class of one row: variance 0 (+ epsilon)
            assert all(v == 0 for v in ex['V'][cls])


def test_the_split_sits_on_the_block_edge_from_both_sides():
    # t < n0 decides the class of row t: n0 = 512 makes lane 0's second row the first of class 1, n0 = 513 its last of class 0
    assert NC.CASES['rows_1025_n0_512']['expect'] == dict(n1=513, one_row_class=False, strides0=1, strides1=2)
    assert NC.CASES['rows_1025_n0_513']['expect'] == dict(n1=512, one_row_class=False, strides0=2, strides1=1)


@pytest.mark.parametrize('name', sorted(n for n, c in NC.CASES.items() if c['edge'] == 'width'))
def test_width_cases_sit_around_the_pairwise_switch(name):
    c = NC.CASES[name]
    assert c['expect']['pairwise'] == (c['d'] >= 8)
    assert c['expect']['tail'] == (c['d'] % 8 if c['d'] >= 8 else c['d'])


@pytest.mark.parametrize('name', sorted(n for n, c in NC.CASES.items() if c['edge'] == 'column'))
def test_column_cases_are_what_a_careless_variance_gets_wrong(name):
    c = NC.CASES[name]
    X, y, [(tr, va)] = NC.problem(c)
    [ex] = NC.exact(c)
    for cls, f in c['expect'].get('zero_var', ()):
        assert ex['V'][cls][f] == 0
    Xt, yt = X[tr], y[tr]
    if c['kind'] == 'const_col':
        assert np.ptp(Xt[:, 0]) == 0 and Fraction(float(Xt[0, 0])).denominator > 2 ** 40      # (its multiples are not all floats)
    if c['kind'] == 'const_in_class':
        assert np.ptp(Xt[yt == 0, 0]) == 0 and np.ptp(Xt[yt == 1, 0]) > 0
    if c['kind'] == 'far_mean':
        for cls in (0, 1):
            col = Xt[yt == cls, 0]
            if len(col) > 1:
                onepass = float(np.mean(col * col) - np.mean(col) ** 2)  # what a one-pass variance would give
                assert abs(onepass - float(ex['V'][cls][0])) > 1e6 * float(ex['W'][cls][0])
                assert float(ex['M'][cls][0]) > 1e10 * float(ex['V'][cls][0]) ** 0.5
    if c['kind'] == 'var_scales':
        for cls in (0, 1):
            assert 0.5e-8 < float(ex['V'][cls][0]) < 2e-8 and 7 < float(ex['V'][cls][1]) < 11
            # the existing acceptance (1e-12 of the largest variance) is a relative 1e-4 and more on column 0
            assert 1e-12 * float(max(ex['V'][cls])) > 1e8 * float(ex['W'][cls][0])


def test_the_bound_is_the_one_derived():
    assert [NC.chain(m) for m in (1, 512, 513, 1024, 1025)] == [15, 15, 16, 16, 17]
    assert [NC.k_prime(m) for m in (1, 512, 513, 1024, 1025)] == [19, 19, 20, 20, 21]
    assert NC.g(19) == Fraction(19, 2 ** 53 - 19)
