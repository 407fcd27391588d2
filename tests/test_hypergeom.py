"""mc_hypergeom.h, the host build (mc_hypergeom_tail, mc_hypergeom_tail_many, mc_hypergeom_round4, mc_hypergeom_tie4): the
hypergeometric tail of evaluate.py's subsampled-depth tables against exact rationals, its DERIVED bound against the error that is
there, the trivial cases, np.round(., 4) restated, the tie test -- and the figures on record in profiles/hypergeom_error.json."""
import json
import math
import os
from fractions import Fraction

import numpy as np

from tests import helpers as H
from tests import hypergeom_grid as G


def test_tail_is_within_its_derived_bound_of_the_exact_tail_on_the_grid():
    from mcaller_amd import _lib
    N, K, d, k, exact = G.cases()
    assert len(N) > 15000 and d.max() == 2000 and (d == N).any() and (K == 0).any() and (K == N).any()
    tail, err = _lib.hypergeom_tail(N, K, d, k)
    worst, worst_bound, at = 0.0, 0.0, None
    for i, (num, den) in enumerate(exact):
        assert G.within(tail[i], err[i], num, den), (N[i], K[i], d[i], k[i], tail[i], err[i])
        e = G.abs_error(tail[i], num, den)
        if e > worst:
            worst, at = e, i
        worst_bound = max(worst_bound, err[i])
    print('largest |tail - exact| %.3g at (N, K, d, k) = %s; largest derived bound %.3g' % (worst, (N[at], K[at], d[at], k[at]) if at is not None else None, worst_bound))
    assert (tail >= 0.0).all() and (tail <= 1.0).all()
    # the bound says something: far below what the tie test of four decimals has to tell apart
    assert worst_bound < 2e-12
    # a walk that stops below 2^-900 took part, and its bound still holds (asserted above)
    deep = (N == 2000) & (d == 1024) & (K == 1000)
    assert deep.any() and (tail[deep] < 1e-200).any()


def test_the_trivial_cases_are_exact():
    from mcaller_amd import _lib
    for N, K, d in ((1, 0, 1), (1, 1, 1), (10, 3, 4), (10, 7, 5), (30, 30, 7), (30, 0, 7), (1500, 700, 1024), (5, 2, 0)):
        lo, hi = max(0, d - (N - K)), min(K, d)
        for k in (-3, 0, lo):
            assert _lib.hypergeom_tail(N, K, d, k) == (0, 1.0, 0.0), (N, K, d, k)
        for k in (hi + 1, d + 1, d + 50):
            assert _lib.hypergeom_tail(N, K, d, k) == (0, 0.0, 0.0), (N, K, d, k)
    # d == N: the draw is the site, the tail is 0 or 1
    assert _lib.hypergeom_tail(12, 5, 12, 5) == (0, 1.0, 0.0) and _lib.hypergeom_tail(12, 5, 12, 6) == (0, 0.0, 0.0)
    # one draw: K / N
    st, t, e = _lib.hypergeom_tail(7, 3, 1, 1)
    assert st == 0 and abs(t - 3 / 7) <= e and 0 < e < 1e-14
    for bad in ((-1, 0, 0, 0), (5, 6, 1, 1), (5, 2, 6, 1), (5, -1, 2, 1), (5, 2, -1, 0), (1 << 31, 5, 2, 1), (1 << 22, 5, (1 << 20) + 1, 1)):
        st, t, e = _lib.hypergeom_tail(*bad)
        assert st == 1 and math.isnan(t) and math.isnan(e), bad
    tail, err = _lib.hypergeom_tail([5, 5], [6, 2], [1, 2], [1, 1])
    assert np.isnan(tail[0]) and np.isnan(err[0]) and abs(tail[1] - 0.7) <= err[1]
    assert _lib.hypergeom_tail([], [], [], [])[0].shape == (0,)


def test_large_arguments_stay_exact_integers():
    """N near 2^31 with d = 1024: every product of the recurrence is below 2^53, and the bound holds against the exact tail."""
    from mcaller_amd import _lib
    N, d = (1 << 31) - 1, 1024
    for K in (1, 1000, N // 3, N - 5):
        num, den = G.tail_numerators(N, K, d)
        for k in (1, 2, 300, 341, 342, 400, 1024):
            st, t, e = _lib.hypergeom_tail(N, K, d, k)
            assert st == 0 and G.within(t, e, num[k], den), (K, k, t, e)


def test_round4_is_np_round():
    from mcaller_amd import _lib
    rng = np.random.RandomState(17)
    v = np.concatenate([rng.uniform(0, 1, 50000), rng.randint(0, 10000, 30000) / 10000.0 + 0.00005, rng.randint(0, 10001, 15000) / 10000.0,
                        rng.normal(0, 3, 4000),
                        [0.00005, 0.00015, 0.00025, -0.00005, 0.03125, 0.5, 1.0, 0.0, -0.0, 1e-9, -1e-9, 0.99995, 0.99994999, float('nan')] + [0.25] * 986])
    assert len(v) == 100000
    got = np.array([_lib.hypergeom_round4(x) for x in v])
    want = np.round(v, 4)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all() and (np.signbit(got) == np.signbit(want)).all()
    assert str(np.float64(_lib.hypergeom_round4(0.03125))) == '0.0312' and str(np.float64(_lib.hypergeom_round4(-0.00004))) == '-0.0'


def test_tie4():
    from mcaller_amd import _lib
    tie = _lib.hypergeom_tie4
    assert not tie(0.12344, 1e-9) and not tie(0.12344, 9e-6) and tie(0.12344, 1.1e-5)
    assert tie(0.03125, 1e-15) and tie(0.03125, 0.0) is False                     # 1/32 is a double: alone it rounds one way
    assert tie(0.12345, 1e-15) and tie(np.nextafter(0.12345, 1), 1e-12) and not tie(0.12345 + 1e-9, 1e-12)
    assert tie(1e-9, 2e-9) and not tie(1e-9, 5e-10)                                # -0.0 against 0.0: another text
    assert not tie(0.5, 1e-12) and not tie(1.0, 1e-12) and not tie(0.0, 0.0)
    assert tie(float('nan'), 0.0) and tie(0.5, float('nan')) and tie(0.5, float('inf'))


def test_the_recorded_figures():
    """profiles/hypergeom_error.json: what tools/hypergeom_error.py measured lies under the derived bound it found beside it."""
    rec = json.load(open(os.path.join(H.REPO, 'profiles', 'hypergeom_error.json')))
    host = rec['host']
    assert host['cases'] > 10 ** 6 and host['violations'] == 0
    assert 0.0 < host['measured_max'] <= host['derived_err_max'] < 2e-12
    if rec.get('device'):
        dev = rec['device']
        assert dev['violations'] == 0 and 0.0 < dev['measured_max'] <= dev['derived_err_max'] < 2e-12
    # the exact side of the tool and of this file agree on a case worked by hand: C(4, 2) = 6 draws, 5 with a marked read
    num, den = G.tail_numerators(4, 2, 2)
    assert (num, den) == ([6, 5, 1, 0], 6) and Fraction(num[1], den) == Fraction(5, 6)
