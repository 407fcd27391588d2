"""compare_currents on the host: the host statement against an independent restatement (plain dict loops, direct SciPy calls per
column), written-out lines with every error and edge of the definition, --fdr against false_discovery_control, --sig_bed through
find_motifs, and mc_curcombine.h's host build (mc_curcombine) against the Python statement with its tie status checked both ways."""
import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import compare_currents as CC
from tests import currents_cases as K


def run(tmp_path, native, control, **kw):
    p1, p2 = K.files(tmp_path, native, control)
    out, bed = str(tmp_path / 'out.tsv'), str(tmp_path / 'sig.bed')
    want_bed = kw.pop('want_bed', False)
    n = CC.compare_currents(p1, p2, out=out, sig_bed=bed if want_bed else None, **kw)
    return open(out, 'rb').read(), (open(bed, 'rb').read() if want_bed else None), n


@pytest.mark.parametrize('fdr', [False, True])
def test_host_statement_against_the_brute_force(tmp_path, fdr):
    native, control = K.seeded_pair(12, 4, 22, seed=11)
    for depth, by in ((4, 'mwu'), (15, 'ks')):
        rows, bed, n = run(tmp_path, native, control, depth=depth, fdr=fdr, by=by, threshold=1.0, want_bed=True)
        want_rows, want_bed, _ = K.brute_rows(native, control, depth, fdr, by, 1.0)
        assert rows == want_rows and bed == want_bed
        assert n == rows.count(b'\n') and CC.last_compare == dict(by='host', reason='the host statement was asked for', n_sites=n, n_sig=bed.count(b'\n'))
        assert depth == 15 or 0 < bed.count(b'\n') < n
    assert 0 < K.brute_rows(native, control, 15)[0].count(b'\n') < 12 == K.brute_rows(native, control, 4)[0].count(b'\n')


def test_written_out_lines(tmp_path):
    x = [[0.1, 0.5], [0.3, -0.2], [-0.4, 0.9]]
    y = [[1.1, 0.4], [1.4, -0.1], [0.9, 0.8]]
    native = ''.join(K.row('chr1', 10, '+', v, prob=None if i == 1 else 0.5, read='a%d' % i) for i, v in enumerate(x)) + \
        K.row('chr1', 10, '-', x[0]) + K.row('chr9', 3, '+', x[0]) * 3
    control = K.row('chrZ', 1, '+', y[0]) + ''.join(K.row('chr1', 10, '+', v, read='b%d' % i, context='TTTTMTTTTTT') for i, v in enumerate(y))
    rows, _, n = run(tmp_path, native.encode(), control.encode(), depth=3)
    assert n == 1
    f = rows.decode().rstrip('\n').split('\t')
    assert f[:7] == ['chr1', '10', '11', 'GATCMGATCGA', '+', '3', '3'] and len(f) == 7 + 2 + 4
    from scipy.stats import ttest_ind
    assert f[7:9] == [str(np.round(ttest_ind([v[j] for v in x], [v[j] for v in y]).statistic, 3)) for j in (0, 1)]
    assert rows == K.brute_rows(native.encode(), control.encode(), 3)[0]
    # the -d edge: n = d - 1 in either file is no site, n = d is one
    assert run(tmp_path, native.encode(), control.encode(), depth=4)[2] == 0
    assert run(tmp_path, (native + K.row('chr1', 10, '+', [0.2, 0.2])).encode(), control.encode(), depth=4)[2] == 0
    assert run(tmp_path, (native + K.row('chr1', 10, '+', [0.2, 0.2])).encode(), (control + K.row('chr1', 10, '+', [1.0, 0.3])).encode(), depth=4)[2] == 1
    # a last line without its newline, in either file
    assert run(tmp_path, native.encode()[:-1], control.encode()[:-1], depth=3)[0] == rows
    with pytest.raises(ValueError, match='-d is at least 2'):
        run(tmp_path, native.encode(), control.encode(), depth=1)


def test_every_value_error_names_file_and_line(tmp_path):
    good = K.row('chr1', 10, '+', [0.1, 0.5])
    cases = {'fields_6': (good + 'chr1\tr\t10\tGATC\t0.1,0.2,9.0\t+\n', 'line 2: 6 tab-separated fields'),
             'fields_9': (good + good.rstrip('\n') + '\t0.5\tx\n', 'line 2: 9 tab-separated fields'),
             'empty line': (good + '\n' + good, 'line 2: 1 tab-separated fields'),
             'number': (good + good.replace('0.5', '0.5x'), 'line 2: a value that is no number'),
             'quality': (good + good.replace('9.5', ''), 'line 2: a value that is no number'),
             'count': (good + K.row('chr1', 10, '+', [0.1, 0.5, 0.7]), 'line 2: 4 values, 3 are expected'),
             'pos': (good + good.replace('\t10\t', '\t1o\t'), 'line 2: a position that is no integer')}
    for name, (text, message) in cases.items():
        for which in (0, 1):
            native, control = (text, good) if which == 0 else (good, text)
            with pytest.raises(ValueError, match='%s.diffs.6 %s' % (('native', 'control')[which], message)):
                run(tmp_path, native.encode(), control.encode(), depth=2)
    with pytest.raises(ValueError, match='native.diffs.6 line 1: 1 values, at least 2 are needed'):
        run(tmp_path, b'chr1\tr\t10\tGATC\t9.0\t+\tA\n', good.encode(), depth=2)
    assert run(tmp_path, b'', good.encode(), depth=2) == (b'', None, 0)


def test_bonferroni_clamp_and_equal_means(tmp_path):
    """Two samples from one distribution: every column's -log10 p is below log10 c and the row prints 0.0; a column with equal
    means prints t = 0.0 (never -0.0)."""
    x = np.asarray([[0.1, 0.1], [0.4, 0.5], [0.8, 0.2], [0.35, 0.3], [0.6, 0.9], [0.45, 0.4]])
    y = np.asarray([[0.45, 0.15], [0.45, 0.45], [0.2, 0.25], [0.7, 0.35], [0.3, 0.8], [0.6, 0.4]])
    assert np.mean(x[:, 0]) == np.mean(y[:, 0])
    native = ''.join(K.site_lines('chr1', 5, '+', x, 'n')).encode()
    control = ''.join(K.site_lines('chr1', 5, '+', y, 'c')).encode()
    rows, _, n = run(tmp_path, native, control, depth=6, fdr=True)
    f = rows.decode().rstrip('\n').split('\t')
    _, logs = K.brute_logs(x, y)
    assert n == 1 and all(-min(col) < np.log10(2) for col in logs)
    assert f[7] == '0.0' and f[9:] == ['0.0'] * 8


def test_fdr_against_scipy(tmp_path):
    from scipy.stats import false_discovery_control
    native, control = K.seeded_pair(40, 5, 9, seed=13, planted=2)
    rows, _, n = run(tmp_path, native, control, depth=5, fdr=True)
    _, _, L = K.brute_rows(native, control, 5)
    assert n == 40 == len(L)
    got = np.asarray([[float(v) for v in line.split('\t')[-4:]] for line in rows.decode().splitlines()])
    from mcaller_amd.compare_genomes import bh_log10
    for i in range(4):
        q = false_discovery_control(10.0 ** L[:, i])
        worst = float(np.max(np.abs(10.0 ** bh_log10(L[:, i]) - q) / q))
        print('column %d: largest relative difference of q to false_discovery_control: %.3g' % (i, worst))
        assert worst <= 1.4e-15
        assert np.all(np.abs(got[:, i] - (0.0 - np.log10(q))) <= 0.0005 + 1e-12)
    assert len(set(got[:, 0])) > 3


def test_sig_bed_is_accepted_by_find_motifs(tmp_path):
    from mcaller_amd import find_motifs as FM
    native, control = K.seeded_pair(12, 6, 10, seed=17, planted=2)
    rows, bed, n = run(tmp_path, native, control, depth=6, by='t', threshold=1.5, want_bed=True)
    lines = bed.decode().splitlines()
    assert 0 < len(lines) < n == 12 and all(len(l.split('\t')) == 7 for l in lines)
    by_key = {tuple(r.split('\t')[:3]): r.split('\t') for r in rows.decode().splitlines()}
    for l in lines:
        f = l.split('\t')
        r = by_key[tuple(f[:3])]
        assert f == r[:4] + [r[7 + K.C6 + 2], r[4], r[5]] and float(f[4]) >= 1.5
    assert sum(float(r[7 + K.C6 + 2]) >= 1.5 for r in by_key.values()) == len(lines)
    path = str(tmp_path / 'sig.bed')
    ref = {'chr1': 'A' * 400}
    listed = FM.read_sites(path, ref)
    assert int(listed['chr1'][0].sum() + listed['chr1'][1].sum()) == len(lines)


def statement(L, log10c):
    with np.errstate(all='ignore'):
        v = np.minimum(0.0, np.min(L) + log10c)
        return v, np.round(0.0 - v, 3)


def test_curcombine_against_the_statement():
    u = 2.0 ** -53
    rng = np.random.default_rng(19)
    n_tie = 0
    for k in range(10000):
        c = int(rng.integers(1, 13))
        log10c = float(np.log10(c))
        L = -(10.0 ** rng.uniform(-6, 2.4, size=c))
        if k % 7 == 0:
            L[int(rng.integers(0, c))] = -0.0 if k % 14 else -1e-9 * rng.random()      # the clamp: p = 1 in a column
        bound = 10.0 ** rng.uniform(-16, -12, size=c) * np.maximum(1.0, -L)
        out, rounded, b, st = _lib.curcombine(L, bound, log10c)
        want, want_rounded = statement(L, log10c)
        assert out == want
        assert str(rounded) == str(want_rounded)
        s = np.min(L) + log10c
        e = np.max(bound) + 2 * u * (abs(s) + np.max(bound))
        if s - e > 0.0:
            assert (out, b, rounded, st) == (0.0, 0.0, 0.0, 0)                          # clamped on both sides: exact
            continue
        assert b == e
        lo, hi = max(0.0, (0.0 - out) - e), max(0.0, (0.0 - out) + e)
        tie = np.round(lo, 3) != np.round(hi, 3)
        assert st == (_lib.CC_STATUS['tie'] if tie else 0), (L, bound, st)
        n_tie += tie
        if s >= 0.0:
            assert rounded == 0.0 and st == 0                                           # a clamp never declines
    print('random vectors on a tie: %d' % n_tie)
    # crafted: the sum inside, and just outside, its bound of a three-decimal tie
    for k in range(2000):
        c = int(rng.integers(1, 9))
        log10c = float(np.log10(c))
        tie_at = (int(rng.integers(0, 290000)) + 0.5) / 1000.0
        b = 10.0 ** rng.uniform(-13, -9) * max(1.0, tie_at)                  # (hundreds of ulps of the value: the test's own roundings are far inside)
        for factor, want_tie in ((0.5, True), (-0.5, True), (1.5, False), (-1.5, False)):
            L = -rng.uniform(0.0, tie_at, size=c) * 0.5 - log10c
            L[int(rng.integers(0, c))] = -(tie_at + factor * b) - log10c
            L = np.minimum(L, 0.0)
            out, rounded, e, st = _lib.curcombine(L, np.full(c, b), log10c)
            assert out == statement(L, log10c)[0] and b <= e <= b * 1.01
            assert st == (_lib.CC_STATUS['tie'] if want_tie else 0), (tie_at, b, factor, st)


def test_curcombine_statuses():
    nan = float('nan')
    assert _lib.curcombine([-1.0, nan], [0.0, 0.0], 0.3)[3] == _lib.CC_STATUS['nan']
    assert _lib.curcombine([-1.0, 0.5], [0.0, 0.0], 0.3)[3] == _lib.CC_STATUS['range']
    assert _lib.curcombine([-1.0, -np.inf], [0.0, 0.0], 0.3)[3] == _lib.CC_STATUS['range']
    assert _lib.curcombine([-1.0], [-1e-9], 0.0)[3] == _lib.CC_STATUS['range']
    assert _lib.curcombine([-1.0], [np.inf], 0.0)[3] == _lib.CC_STATUS['range']
    out, rounded, b, st = _lib.curcombine([-1.2345, -0.5], [1e-9, 0.0], 0.0)
    assert (out, st) == (-1.2345, _lib.CC_STATUS['tie']) and rounded in (1.234, 1.235)
    assert _lib.curcombine([-1.2341, -0.5], [1e-9, 0.0], 0.0)[1:] == (1.234, 1e-9 + 2 * 2.0 ** -53 * (1.2341 + 1e-9), 0)
    with pytest.raises(ValueError):
        _lib.curcombine([], [], 0.0)


def test_the_command_line_and_the_shim(tmp_path, capsys):
    import os
    import subprocess
    import sys
    from tests import helpers as H
    native, control = K.seeded_pair(3, 4, 6, seed=23)
    p1, p2 = K.files(tmp_path, native, control)
    out, bed = str(tmp_path / 'o.tsv'), str(tmp_path / 'o.bed')
    CC.main(['--native', p1, '--control', p2, '-d', '4', '--fdr', '--sig_bed', bed, '--by', 'rs', '--threshold', '0.5', '-o', out])
    want = K.brute_rows(native, control, 4, True, 'rs', 0.5)
    assert (open(out, 'rb').read(), open(bed, 'rb').read()) == want[:2]
    for d in ('0', '1'):
        with pytest.raises(SystemExit):
            CC.main(['--native', p1, '--control', p2, '-d', d])
    capsys.readouterr()
    got = subprocess.run([sys.executable, os.path.join(H.REPO, 'compare_currents.py'), '--native', p1, '--control', p2, '-d', '4'],
                         capture_output=True, check=True).stdout
    assert got == K.brute_rows(native, control, 4)[0]
