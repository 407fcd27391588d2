"""mc_hypergeom.h's hg_masses, the host build (mc_hypergeom_masses, mc_hypergeom_masses_many): the bucket masses behind all 101
tails of a (N, K, d) against exact rationals on the grid of tests/hypergeom_grid.py, reduced to its distinct (N, K, d) -- every
tail formed from the masses EXACTLY (a sum of doubles as a rational) lies within the one derived bound; the cases of one value."""
from fractions import Fraction

import numpy as np

from tests import hypergeom_grid as G

_shapes = None


def shapes():
    """The distinct (N, K, d) of the grid -> int64 arrays N, K, d."""
    global _shapes
    if _shapes is None:
        N, K, d, _, _ = G.cases()
        _shapes = tuple(np.ascontiguousarray(a) for a in np.unique(np.stack([N, K, d], axis=1), axis=0).T)
    return _shapes


def check_masses(N, K, d, mass, err, km_of):
    """Every tail_j = sum_{c > j} mass[c] within err of num[k_min(d, j)] / den, decided in integers -> the largest err seen."""
    worst = 0.0
    for i in range(len(N)):
        n, k, dd = int(N[i]), int(K[i]), int(d[i])
        num, den = G.tail_numerators(n, k, dd)
        km = km_of(dd)
        m = mass[i]
        assert m[0] == 0.0 and (m >= 0.0).all() and (m <= 1.0).all(), (n, k, dd)
        lo, hi = max(0, dd - (n - k)), min(k, dd)
        if lo == hi:
            assert err[i] == 0.0 and sorted(m)[-2:] == [0.0, 1.0] and m[(100 * lo) // dd + 1] == 1.0, (n, k, dd)
        tail = Fraction(0)                                    # exact: the doubles as rationals
        for j in range(100, -1, -1):
            tail += Fraction(float(m[j + 1]))
            a, b = tail.numerator, tail.denominator           # |a / b - num / den| <= err  <=>  |0 - (num b - a den) / (den b)| <= err
            assert G.within(0.0, err[i], num[km[j]] * b - a * den, den * b), (n, k, dd, j, float(tail), err[i])
        worst = max(worst, float(err[i]))
    return worst


_km = {}


def k_min(d):
    from mcaller_amd import evaluate
    if d not in _km:
        _km[d] = evaluate.k_min(d)
    return _km[d]


def test_every_tail_from_the_masses_is_within_the_derived_bound_on_the_grid():
    from mcaller_amd import _lib
    N, K, d = shapes()
    assert len(N) > 1000 and d.max() == 2000 and (d == N).any() and (K == 0).any() and (K == N).any() and (d == 1024).any()
    mass, err = _lib.hypergeom_masses(N, K, d)
    assert mass.shape == (len(N), 102)
    worst = check_masses(N, K, d, mass, err, k_min)
    print('largest derived bound %.3g over %d shapes' % (worst, len(N)))
    assert 0.0 < worst < 2e-12                                 # far below what the tie test of four decimals has to tell apart
    # the masses and hg_tail tell one story: the tail at k_min(d, j) within the sum of the two bounds
    for i in (0, len(N) // 2, len(N) - 1):
        km = k_min(int(d[i]))
        for j in (0, 1, 37, 50, 99, 100):
            st, t, e = _lib.hypergeom_tail(int(N[i]), int(K[i]), int(d[i]), km[j])
            assert st == 0 and abs(float(mass[i][j + 1:].sum()) - t) <= e + err[i] + 102 * 2.0 ** -53


def test_one_value_is_one_bucket_of_mass_one():
    from mcaller_amd import _lib
    for N, K, d in ((1, 0, 1), (1, 1, 1), (12, 5, 12), (30, 30, 7), (30, 0, 7), (2000, 2000, 1024), (2000, 0, 1024), (5, 2, 0)):
        st, mass, err = _lib.hypergeom_masses(N, K, d)
        x = max(0, d - (N - K))
        c = (100 * x) // d + 1 if d else 1
        assert st == 0 and err == 0.0 and mass[c] == 1.0 and mass.sum() == 1.0, (N, K, d)
    # one draw: K / N in bucket 101, the rest in bucket 1
    st, mass, err = _lib.hypergeom_masses(7, 3, 1)
    assert st == 0 and abs(mass[101] - 3 / 7) <= err and abs(mass[1] - 4 / 7) <= err and 0 < err < 1e-14 and mass[2:101].sum() == 0.0


def test_bad_arguments_give_nan():
    from mcaller_amd import _lib
    for bad in ((-1, 0, 0), (5, 6, 1), (5, 2, 6), (5, -1, 2), (5, 2, -1), (1 << 31, 5, 2), (1 << 22, 5, (1 << 20) + 1)):
        st, mass, err = _lib.hypergeom_masses(*bad)
        assert st == 1 and np.isnan(mass).all() and np.isnan(err), bad
    mass, err = _lib.hypergeom_masses([5, 5], [6, 2], [1, 2])
    assert np.isnan(mass[0]).all() and np.isnan(err[0]) and not np.isnan(mass[1]).any() and abs(mass[1][51:].sum() - 0.7) <= err[1] + 1e-15
    assert _lib.hypergeom_masses([], [], [])[0].shape == (0, 102)


def test_the_recorded_figures():
    """profiles/hypergeom_error.json, section `masses`: what tools/hypergeom_error.py --masses measured lies under the derived bound."""
    import json
    import os
    from tests import helpers as H
    rec = json.load(open(os.path.join(H.REPO, 'profiles', 'hypergeom_error.json')))['masses']
    for build in ('host', 'device'):
        if rec.get(build):
            r = rec[build]
            assert r['cases'] > 50000 and r['violations'] == 0 and 0.0 < r['measured_max'] <= r['derived_err_max'] < 2e-12, build
    assert rec['host']
