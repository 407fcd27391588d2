"""compare_genomes --fisher --fdr on the host: mc_fisher.h's host build (mc_fisher_exact) and the host statement (fisher_log10p)
against exact rationals and SciPy, the selection predicate at its factor, bh_log10 against the O(m^2) definition and
false_discovery_control, mc_bh.h's host build (mc_bh_adjust) against bh_log10, and compare_rows with every flag combination."""
import os
from fractions import Fraction

import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import compare_genomes as CG
from tests import fisher_bh_cases as F
from tests import twosample_cases as T

BAD_ARGS, FAR_TAIL, SELECT = (_lib.ABI.constants['MC_FISHER_' + k] for k in ('BAD_ARGS', 'FAR_TAIL', 'SELECT'))
BH_TIE, BH_RANGE = _lib.ABI.constants['MC_BH_TIE'], _lib.ABI.constants['MC_BH_RANGE']
BH_SLACK = 1.0e-13                            # mc_bh.h's derived slack of the terms


def held_against_exact(tables, walked):
    """Every table's log10 p within its own bound of the exact one, every status the expected one -> the largest error and bound."""
    K1, n1, K2, n2 = np.asarray(tables, dtype=np.int64).T
    L, bound, status = _lib.fisher_exact(K1, n1, K2, n2)
    worst_err = worst_bound = 0.0
    for t, l, b, st in zip(tables, L, bound, status):
        p, nearest = F.fisher_p(*t, walked=walked)
        exact = F.log10_exact(p)
        assert abs(abs(nearest / F.FACTOR - 1) - 0) > 1e-8 or nearest == 1, (t, 'a mass at the factor: not a table for this test')
        assert abs(exact - F.FAR_TAIL) > 1e-6, t
        assert st == (FAR_TAIL if exact < F.FAR_TAIL else 0), (t, st, exact)
        assert abs(l - exact) <= b, (t, l, exact, b)
        if p == 1 or min(t[1], t[3]) == 0:
            assert l == 0.0 and (b == 0.0 or p == 1), t
        if np.isfinite(b):
            worst_err, worst_bound = max(worst_err, abs(l - exact)), max(worst_bound, b)
    return worst_err, worst_bound


def test_host_build_on_every_small_table():
    tables = F.small_tables()
    assert len(tables) == 8100
    err, bound = held_against_exact(tables, walked=False)
    assert err <= bound < 1e-13


def test_the_walked_masses_are_the_binomial_ones():
    for t in F.small_tables(7):
        assert F.masses(*t) == F.masses_walked(*t)


def test_host_build_on_deep_tables():
    cases = F.seeded_tables()
    assert 280 <= len(cases) <= 340
    names = {c[0] for c in cases}
    assert names == {'random', 'lo > 0', 'K = 0', 'K = N', 'mirrored', 'deep', 'far tail'}
    assert max(c[2] + c[4] for c in cases) == 8192
    err, bound = held_against_exact([c[1:] for c in cases], walked=True)
    assert err <= bound < 1e-11
    for name, K1, n1, K2, n2 in cases:
        st, l, b = _lib.fisher_exact(K1, n1, K2, n2)
        if name in ('K = 0', 'K = N'):
            assert (st, l, b) == (0, 0.0, 0.0)
        if name == 'far tail':
            assert st == FAR_TAIL
        if name == 'lo > 0':
            assert K1 + K2 > n2
    st, l, b = _lib.fisher_exact(4000, 4000, 0, 4192)         # the observed mass lies below 2^-900 of the mode's: never reached
    assert st == FAR_TAIL and l == -np.inf and b == np.inf


def test_bad_arguments():
    for t in [(-1, 5, 2, 5), (6, 5, 2, 5), (2, 5, 6, 5), (2, 5, -1, 5), (1, 2 ** 20 + 1, 1, 5), (1, 5, 1, 2 ** 31 - 5)]:
        st, l, b = _lib.fisher_exact(*t)
        assert st == BAD_ARGS and np.isnan(l) and np.isnan(b), t
    assert _lib.fisher_exact(0, 0, 0, 0) == (0, 0.0, 0.0)


def test_host_statement_against_scipy():
    """fisher_log10p against scipy.stats.fisher_exact on 3000 seeded tables with n < 80.  A table with a mass ratio in
    (1 + 1e-14, 1 + 1e-7] is left out: SciPy selects by a relative 1e-7 on lgamma-based masses, the definition by the exact ones."""
    from scipy.stats import fisher_exact
    rng = np.random.default_rng(53)
    worst, left_out = 0.0, 0
    for _ in range(3000):
        n1, n2 = (int(v) for v in rng.integers(1, 80, size=2))
        K1, K2 = int(rng.integers(0, n1 + 1)), int(rng.integers(0, n2 + 1))
        lo, w = F.masses(K1, n1, K2, n2)
        if any(1 + Fraction(1, 10 ** 14) < v / w[K1 - lo] <= F.FACTOR for v in w):
            left_out += 1
            continue
        want = fisher_exact([[K1, n1 - K1], [K2, n2 - K2]])[1]
        p, _ = F.fisher_p(K1, n1, K2, n2)
        L = CG.fisher_log10p(K1, n1, K2, n2)
        assert L == F.log10_exact(p), (K1, n1, K2, n2)
        worst = max(worst, abs(float(p) - want) / want)
        assert CG.fisher_nlp(K1, n1, K2, n2) == str(np.round(0.0 - L, 3))
    print('largest relative difference of p to SciPy: %.3g; left out: %d' % (worst, left_out))
    assert left_out <= 30
    assert worst <= 1e-12
    assert CG.fisher_nlp(3, 3, 4, 4) == '0.0' and CG.fisher_log10p(0, 5, 0, 7) == 0.0


def test_selection_predicate_at_its_factor():
    """Ratios placed at 1 + 1e-7 plus or minus the predicate's own error e = gamma(4 S + 8): within e the status says so, beyond it
    the computed selection is the exact one; the exact ties of a symmetric table (ratio 1 to 1e-13) are selected and are not near."""
    u = 2.0 ** -53
    for S in (1.0, 60.0, 4096.0, 2.0 ** 20):
        k = (4 * S + 8) * u
        e = k / (1 - k)
        w_obs = 0.37
        thr = w_obs * 1.0000001
        for factor, selected, near in [(1 - 3 * e, True, False), (1 - 0.5 * e, True, True), (1.0, True, True), (1 + 0.5 * e, False, True),
                                       (1 + 3 * e, False, False)]:
            w = thr * factor
            if (factor != 1.0) and w == thr:
                continue                          # (e below an ulp of thr: nothing lies between)
            assert _lib.fisher_select(w, w_obs, S) == (selected, near), (S, factor)
        for tie in (1.0, 1 - 1e-13, 1 + 1e-13):
            assert _lib.fisher_select(w_obs * tie, w_obs, S) == (True, False), (S, tie)
        assert _lib.fisher_select(w_obs * 1.000001, w_obs, S) == (False, False)
    for n, a, b in [(10, 3, 7), (500, 100, 300), (4096, 1000, 1100)]:            # mirrored tables: the tie is selected, no SELECT
        (st1, l1, _), (st2, l2, _) = _lib.fisher_exact(a, n, b, n), _lib.fisher_exact(b, n, a, n)
        assert st1 == st2 == 0 and l1 == l2


@pytest.mark.parametrize('name', sorted(F.bh_columns()))
def test_bh_log10_is_the_definition(name):
    L = F.bh_columns()[name]
    with np.errstate(all='ignore'):
        Q, want = CG.bh_log10(L), F.bh_brute(L)
    assert np.array_equal(Q, want, equal_nan=True), name
    assert np.array_equal(np.isnan(Q), np.isnan(L))
    if name == 'one row':
        assert Q[0] == L[0]
    if name == 'all equal':
        assert np.all(Q == L[0])
    # equal L, equal Q, and the order of the input does not matter
    perm = np.random.default_rng(3).permutation(len(L))
    assert np.array_equal(CG.bh_log10(L[perm]), Q[perm], equal_nan=True)
    for v in np.unique(L[~np.isnan(L)]):
        assert len(set(Q[L == v])) == 1


def test_bh_log10_against_scipy():
    from scipy.stats import false_discovery_control
    p = np.random.default_rng(59).random(1000) ** 2
    q = 10.0 ** CG.bh_log10(np.log10(p))
    worst = float(np.max(np.abs(q - false_discovery_control(p)) / false_discovery_control(p)))
    print('largest relative difference of q to false_discovery_control: %.3g' % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('name', sorted(F.bh_columns()))
def test_host_build_of_the_adjustment(name):
    L = F.bh_columns()[name]
    bound = np.full(len(L), 1e-15)
    Q, rounded, st = _lib.bh_adjust(L, bound)
    want = CG.bh_log10(L)
    assert np.array_equal(np.isnan(Q), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(Q[ok] - want[ok]) <= BH_SLACK), name
    assert np.array_equal(rounded[ok], np.round(0.0 - Q[ok], 3)) and not np.signbit(rounded[ok]).any()
    if not st & BH_TIE:
        assert [str(v) for v in rounded] == [str(np.round(0.0 - q, 3)) for q in want]


def test_adjustment_statuses():
    Q, rounded, st = _lib.bh_adjust(np.asarray([-1.2345]), np.asarray([1e-9]))
    assert st == BH_TIE and Q[0] == -1.2345
    assert _lib.bh_adjust(np.asarray([-1.2341]), np.asarray([1e-9]))[2] == 0
    assert _lib.bh_adjust(np.asarray([-1.2345, -3.0]), np.asarray([0.0, 1e-9]))[2] == BH_TIE       # the column's bound, not the row's
    for L, b in [([0.5], [0.0]), ([-400.0], [0.0]), ([-1.0], [-1.0]), ([-1.0], [np.inf]), ([-1.0], [np.nan]), ([-np.inf], [0.0])]:
        Q, rounded, st = _lib.bh_adjust(np.asarray(L), np.asarray(b))
        assert st == BH_RANGE and np.isnan(Q).all() and np.isnan(rounded).all()
    Q, rounded, st = _lib.bh_adjust(np.zeros(0), np.zeros(0))
    assert st == 0 and len(Q) == 0


# ---- compare_rows with the flags ----

@pytest.fixture(scope='module')
def beds(tmp_path_factory):
    d = tmp_path_factory.mktemp('fisher_bh')
    t1, t2 = F.counted_pair(F.planted_tables(24))
    t1 += F.counted_line('chr1', 90000, '+', 2, 5).encode()               # a line bed2 lacks
    p1, p2 = str(d / 'a.bed'), str(d / 'b.bed')
    open(p1, 'wb').write(t1)
    open(p2, 'wb').write(t2)
    return p1, p2


def test_columns_of_every_flag_combination(beds):
    p1, p2 = beds
    base, n = CG.compare_rows(p1, p2)
    assert n == 24
    rows = {}
    for fisher, fdr in [(False, False), (True, False), (False, True), (True, True)]:
        blob, n_rows = CG.compare_rows(p1, p2, fisher=fisher, fdr=fdr)
        assert n_rows == n
        rows[fisher, fdr] = [line.split('\t') for line in blob.decode().splitlines()]
        assert {len(r) for r in rows[fisher, fdr]} == {17 + fisher + (4 + fisher) * fdr}
        assert ['\t'.join(r[:17]) for r in rows[fisher, fdr]] == base.decode().splitlines()
    assert CG.compare_rows(p1, p2, fisher=False, fdr=False)[0] == base
    tables = F.planted_tables(24)
    for r, rf, t in zip(rows[True, True], rows[True, False], tables):
        assert r[17] == rf[17] == str(np.round(0.0 - F.log10_exact(F.fisher_p(*t)[0]), 3))
    assert rows[True, True][0][17] == rows[True, True][1][17] == '0.0'                 # K = 0, K = N
    assert rows[True, True][2][17] == rows[True, True][3][17] != '0.0'                 # the mirrored pair
    # the q-value columns: bh_brute over the unrounded logs, column by column in the row's order
    logs = []
    for fields in rows[False, False]:
        key = tuple(fields[:4])
        site = []
        CG.site_values(CG.read_bed(p1)[key][1], CG.read_bed(p2)[key][1], site)
        logs.append(site)
    logs = np.asarray(logs)
    fisher_L = np.asarray([F.log10_exact(F.fisher_p(*t)[0]) for t in tables])
    for c in range(4):
        want = [str(np.round(0.0 - q, 3)) for q in F.bh_brute(logs[:, c])]
        assert [r[17 + c] for r in rows[False, True]] == want == [r[18 + c] for r in rows[True, True]], c
    assert [r[22] for r in rows[True, True]] == [str(np.round(0.0 - q, 3)) for q in F.bh_brute(fisher_L)]


def test_a_frac_that_is_no_count(tmp_path):
    ok1, ok2 = F.counted_pair(F.planted_tables(5))
    bad = F.counted_line('chr1', 50000, '+', 0, 9, frac='0.3333')
    good = F.counted_line('chr1', 50000, '+', 3, 9)
    alone = F.counted_line('chr1', 60000, '+', 0, 9, frac='0.3333')
    p1, p2, out = str(tmp_path / 'a.bed'), str(tmp_path / 'b.bed'), str(tmp_path / 'out.tsv')
    for which, (t1, t2) in enumerate([(ok1 + bad.encode(), ok2 + good.encode()), (ok1 + good.encode(), ok2 + bad.encode())], 1):
        open(p1, 'wb').write(t1)
        open(p2, 'wb').write(t2)
        with pytest.raises(ValueError, match=r'^bed%d line 6: frac is not a count over its reads$' % which):
            CG.compare_rows(p1, p2, fisher=True)
        assert CG.compare_rows(p1, p2)[1] == CG.compare_rows(p1, p2, fdr=True)[1] == 6          # frac is only read under --fisher
    open(p1, 'wb').write(ok1 + alone.encode())                                                 # an unshared line is not looked at
    open(p2, 'wb').write(ok2)
    assert CG.compare_rows(p1, p2, fisher=True)[1] == 5
    assert CG.compare_by_position(p1, p2, out=out, fisher=True, fdr=True) == 5
    assert CG.last_compare == dict(by='host', reason='the host statement was asked for', n_sites=5, fisher=True, fdr=True)
    assert open(out, 'rb').read() == CG.compare_rows(p1, p2, fisher=True, fdr=True)[0]
    CG.main(['--bed1', p1, '--bed2', p2, '-o', out, '--fisher'])
    assert open(out, 'rb').read() == CG.compare_rows(p1, p2, fisher=True)[0] and CG.last_compare['fdr'] is False
    for f, n, K in [('0.5', 4, 2), ('1.0', 7, 7), ('0.0', 3, 0), (str(np.float64(5) / np.float64(13)), 13, 5)]:
        assert CG.site_counts(f, n) == K
    for f, n in [('0.3333', 9), ('1.5', 2), ('-0.5', 2), ('nan', 3), ('x', 3), ('0.5', 0)]:
        assert CG.site_counts(f, n) is None


def test_four_decimal_fracs_keep_working_without_the_flag(tmp_path):
    t1, t2, _ = T.bed_pair(T.depth_pairs(6, seed=61))
    p1, p2 = str(tmp_path / 'a.bed'), str(tmp_path / 'b.bed')
    open(p1, 'wb').write(t1)
    open(p2, 'wb').write(t2)
    base, n = CG.compare_rows(p1, p2)
    blob, _ = CG.compare_rows(p1, p2, fdr=True)
    assert n == 6 and [line.rsplit('\t', 4)[0] for line in blob.decode().splitlines()] == base.decode().splitlines()


def test_the_lifted_rows(tmp_path):
    """--xmfa: the 21 columns stand, the new ones follow; the tables are those of the row's two lines."""
    P, lift, n = F.lifted_files(tmp_path)
    base, n_rows = CG.compare_rows(P['bed1'], P['bed2'], **lift)
    assert n_rows == n >= 3
    blob, _ = CG.compare_rows(P['bed1'], P['bed2'], fisher=True, fdr=True, **lift)
    rows = [line.split('\t') for line in blob.decode().splitlines()]
    assert {len(r) for r in rows} == {27} and ['\t'.join(r[:21]) for r in rows] == base.decode().splitlines()
    sites1, sites2 = CG.read_bed(P['bed1']), CG.read_bed(P['bed2'])
    L = []
    for r in rows:
        ((f1, _), x), ((f2, _), y) = sites1[tuple(r[:4])], sites2[tuple(r[4:8])]
        t = (CG.site_counts(f1, len(x)), len(x), CG.site_counts(f2, len(y)), len(y))
        L.append(F.log10_exact(F.fisher_p(*t)[0]))
        assert r[21] == str(np.round(0.0 - L[-1], 3))
    assert [r[26] for r in rows] == [str(np.round(0.0 - q, 3)) for q in F.bh_brute(L)]
    out = str(tmp_path / 'out.tsv')
    CG.main(['--bed1', P['bed1'], '--bed2', P['bed2'], '--xmfa', P['xmfa'], '--fai1', P['fai1'], '--fai2', P['fai2'], '-o', out, '--fisher', '--fdr'])
    assert open(out, 'rb').read() == blob and CG.last_compare['fisher'] and CG.last_compare['fdr'] and 'n_unaligned' in CG.last_compare
