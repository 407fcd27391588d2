"""mc_tstat.h, the host build (mc_tstat, mc_tstat_round3, mc_tstat_tie, mc_tstat_site): the Student t arithmetic of make_bed -p
against SciPy and NumPy, the tie test on constructed values, the position-set rules restated, and -- for every file the GPU
tests of tests/test_gpu_bed_positions.py compare byte for byte -- that the same arithmetic on the host meets no rounding tie and
no other decline, and prints what make_bed.feature_statistics prints."""
import json
import os
import warnings

import numpy as np
import pytest

from tests import bedpos_files as P
from tests import helpers as H
from tests import tstat_grid as G


def test_log10_p_against_scipy_on_the_grid():
    from mcaller_amd import _lib
    df, t, want = G.grid()
    assert len(df) > 5000 and want.min() < -280 and t.max() > 1e150 and t.min() == 1e-6
    n, mean, var = G.triples(df, t)
    got = np.array([_lib.tstat(a, b, c) for a, b, c in zip(n, mean, var)])
    assert (got[:, 0] == 0).all()
    assert (got[:, 1] == t).all()
    err = G.relative_error(got[:, 2], want)
    print('largest error / max(1, |log10 p|): %.3g at df %g, t %g' % (err.max(), df[err.argmax()], t[err.argmax()]))
    assert err.max() <= G.FN_BOUND / 8
    # the bound on record is at least 64 x what is measured here
    rec = json.load(open(os.path.join(H.REPO, 'profiles', 'tstat_error.json')))
    assert rec['bound'] == G.FN_BOUND and rec['bound'] >= 64 * err.max() and rec['bound'] >= 64 * rec['measured_max']


def test_t_itself_and_the_status_bits():
    from mcaller_amd import _lib
    rng = np.random.RandomState(3)
    from scipy import stats
    for n in (2, 3, 5, 40):
        x = rng.normal(0.3, 2.0, size=n)
        st, t, l = _lib.tstat(n, x.mean(), x.var(ddof=1))
        ref = stats.ttest_1samp(x, 0)
        assert st == 0 and abs(t - ref[0]) <= 1e-13 * abs(ref[0]) and abs(l - np.log10(ref[1])) <= 1e-12
    assert _lib.tstat(1, 2.0, 0.0)[0] == 1 and np.isnan(_lib.tstat(1, 2.0, 0.0)[1])
    assert _lib.tstat(3, 2.0, 0.0)[0] == 2 and _lib.tstat(3, 2.0, float('nan'))[0] == 2 and _lib.tstat(3, float('inf'), 1.0)[0] == 2
    assert _lib.tstat(100, 1e6, 1e-12)[0] == 4                 # log10 p far below -290
    assert _lib.tstat(3, 0.0, 1.0)[1:] == (0.0, 0.0)


def test_round3_is_np_round():
    from mcaller_amd import _lib
    rng = np.random.RandomState(11)
    v = np.concatenate([rng.normal(0, 50, 40000), rng.uniform(-1, 1, 30000), rng.randint(-20000, 20000, 29000) / 1000.0 + 0.0005,
                        [0.0005, 0.0015, -0.0005, 0.0025, -0.0015, 0.0, -0.0, 1e-9, -1e-9, 123456.7895, 2.5e-4, -4.9999e-4] + [0.0] * 988])
    assert len(v) == 100000
    got = np.array([_lib.tstat_round3(x) for x in v])
    want = np.round(v, 3)
    assert (got == want).all() and (np.signbit(got) == np.signbit(want)).all()
    assert str(np.float64(_lib.tstat_round3(-0.0004))) == '-0.0'


def test_tie_test():
    from mcaller_amd import _lib
    tie = _lib.tstat_tie
    assert not tie(1.2344, 1e-9) and not tie(1.2344, 9e-5) and tie(1.2344, 1.1e-4)
    assert tie(1.2345, 1e-15) and tie(0.0005, 0.0) is False and tie(0.0005, 1e-20) is False and tie(0.0005, 1e-16)
    assert tie(np.nextafter(1.2345, 2), 1e-12) and not tie(1.2345 + 1e-9, 1e-12)
    assert tie(-3.0005, 1e-13) and not tie(-3.0004, 1e-13)
    assert tie(1e-9, 2e-9) and not tie(1e-9, 5e-10)            # -0.0 against 0.0: another text
    assert not tie(-1e-5, 1e-9)
    assert tie(float('nan'), 0.0) and tie(1.0, float('nan')) and tie(1.0, float('inf'))
    assert not tie(123.0, 0.0)


def _entries(tmp, text, ptext):
    """-> the feature rows of every entry make_bed writes for (text, positions text), in its order."""
    from mcaller_amd import make_bed
    (tmp / 'x.diffs.6').write_bytes(text)
    (tmp / 'x.positions').write_bytes(ptext)
    wanted = make_bed.wanted_positions(str(tmp / 'x.positions'))
    rows = make_bed.read_diffs(str(tmp / 'x.diffs.6'), wanted)
    return rows.features


def _check_files(tmp, files):
    from mcaller_amd import _lib, make_bed
    n_checked = 0
    for name, text, ptext in files:
        for feats in _entries(tmp, text, ptext):
            X = np.asarray(feats, dtype=np.float64)
            st, a, b = _lib.tstat_site(np.hstack([X, np.zeros((len(X), 1))]))
            if len(X) < 2:
                assert st == 1, name
                continue
            assert st == 0, (name, st)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                want = [str(v) for v in make_bed.feature_statistics(feats)]
            assert [str(np.float64(a)), str(np.float64(b))] == want, name
            n_checked += 1
    return n_checked


def test_the_host_build_meets_no_tie_on_the_edge_files(tmp_path):
    files = [(name, text, ptext) for name, (text, ptext, _) in sorted(P.edge_cases().items())]
    assert _check_files(tmp_path, files) > 100


def test_the_host_build_meets_no_tie_on_the_random_files(tmp_path):
    files = [(seed,) + P.random_case(seed)[:2] for seed in range(P.SEED_BASE, P.SEED_BASE + P.N_RANDOM)]
    assert _check_files(tmp_path, files) > 300


def test_the_declines_of_the_decline_files(tmp_path):
    """What the GPU test expects the device to decline for an entry, the host build declines too (its status bits)."""
    from mcaller_amd import _lib
    bits = {20: 2, 21: 4, 22: 64, 23: 16, 24: 32}
    for name, (text, ptext, _, reason, line) in sorted(P.decline_cases().items()):
        if reason in bits:
            feats = [f for f in _entries(tmp_path, text, ptext) if len(f) >= 2]
            sts = [_lib.tstat_site(np.hstack([np.asarray(f), np.zeros((len(f), 1))]))[0] for f in feats]
            assert len([s for s in sts if s]) == 1 and max(sts) & bits[reason], (name, sts)


def test_position_set_rules(tmp_path):
    """make_bed.wanted_positions: len(line) > 3 with the newline, strip, the first four fields, doubles collapse."""
    from mcaller_amd import make_bed
    p = tmp_path / 'p.txt'
    p.write_bytes(b'ab\n\nabc\n  c\t1\t2\t+  \nc\t1\t2\t+\textra\nc\t1\t2\nc\t1\t2\t+\nabc')
    assert make_bed.wanted_positions(str(p)) == {('abc',), ('c', '1', '2', '+'), ('c', '1', '2')}
    p.write_bytes(b'')
    assert make_bed.wanted_positions(str(p)) == set()
    for name, (text, ptext, _) in P.edge_cases().items():
        p.write_bytes(ptext)
        want = set()
        for line in ptext.decode('ascii').split('\n'):
            # (the last piece has no newline behind it)
            pass
        pieces = ptext.decode('ascii').split('\n')
        for i, line in enumerate(pieces):
            full = line + ('\n' if i < len(pieces) - 1 else '')
            if len(full) > 3:
                want.add(tuple(full.strip(' \t\n').split('\t')[:4]))
        assert make_bed.wanted_positions(str(p)) == want, name
