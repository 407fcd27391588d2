"""mcaller_amd.evaluate, the host statement: its bytes against the brute-force restatement of tests/evaluate_cases.py (every
subset of a site's reads enumerated), the `read` AUC against scikit-learn's, the fp64 rule of k_min, empty classes, the depths'
edges, the errors, the command line, and the reference's own test data."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import evaluate_cases as EC
from tests import helpers as H

TESTDATA = os.path.join(H.GOLDEN, 'testdata')


@pytest.mark.parametrize('seed,on_grid', [(1, True), (2, True), (3, False), (4, False)])
def test_host_statement_is_the_brute_force_restatement(seed, on_grid):
    from mcaller_amd import evaluate as E
    diffs, positions = EC.random_case(seed, on_grid=on_grid)
    for min_depth, depths in ((3, (1, 2, 3, 5, 10)), (1, (1, 4, 7, 9)), (11, (2,))):
        want, _ = EC.brute_force(diffs, positions, min_depth, depths)
        got = E.evaluate_calls(diffs, positions, min_depth, depths)
        assert got == want, [(a, b) for a, b in zip(got.split(b'\n'), want.split(b'\n')) if a != b][:5]
    lines = got.decode().split('\n')
    assert lines[0] == E.HEADER and len(lines) == 1 + 101 * 3 + 3 + 1 and lines[-1] == ''
    assert E.last_eval['by'] == 'host' and E.last_eval['n_rows'] == E.last_eval['n_kept'] + 6 + 2
    assert (E.last_eval['n_unlabelled'], E.last_eval['n_not_m']) == (6, 2)
    assert E.last_eval['n_sites'] == E.last_eval['n_pos_sites'] + E.last_eval['n_neg_sites'] == 14


def test_paths_and_bytes_give_the_same_bytes(tmp_path):
    from mcaller_amd import evaluate as E
    diffs, positions = EC.random_case(5)
    (tmp_path / 'a.diffs.6').write_bytes(diffs)
    (tmp_path / 'p.txt').write_bytes(positions)
    assert E.evaluate_calls(str(tmp_path / 'a.diffs.6'), str(tmp_path / 'p.txt'), 2, (1, 3)) == E.evaluate_calls(diffs, positions, 2, (1, 3))


def test_read_auc_is_scikit_learns_on_on_grid_probabilities():
    """mCaller prints np.round(p, 2): every score is a threshold, so the 101-point trapezoid is the Mann-Whitney AUC with ties."""
    from sklearn.metrics import roc_auc_score
    from mcaller_amd import evaluate as E
    rng = np.random.RandomState(8)
    sites, y, s = [], [], []
    for i in range(60):
        positive = i % 3 != 0
        p = np.round(np.clip(rng.normal(0.6 if positive else 0.4, 0.2, rng.randint(1, 30)), 0, 1), 2)
        probs = [str(v) for v in p]
        sites.append(('c', 10 + i, '+', 'm6A' if positive else 'A', [int(v >= 0.5) for v in p], probs))
        y += [int(positive)] * len(p)
        s += [float(t) for t in probs]
    diffs, positions = EC.build(sites, shuffle_seed=3)
    tables = E.evaluate_tables(diffs, positions, 5, (1,))
    assert tables[0]['level'] == 'read' and tables[0]['n_pos'] == sum(y) and len(set(s)) > 50
    assert abs(tables[0]['auc'] - roc_auc_score(y, s)) <= 1e-12
    # the site table's score K / N is no threshold in general: its AUC is the 101-point curve's, not Mann-Whitney's
    assert 0.5 < tables[1]['auc'] <= 1.0


def test_k_min_at_100_7_and_on_every_depth():
    """k_min is defined by the fp64 comparison x / d >= j / 100.  Both quotients are correctly rounded, so equal rationals give
    equal doubles -- at (d, j) = (100, 7): 7 / 100 >= thr[7] holds and k_min is 7 -- and unequal ones are at least 1 / (100 d)
    apart, far more than an ulp: for every d up to 1024 the fp64 rule IS the rule of the rationals.  The test holds both."""
    from mcaller_amd import evaluate as E
    thr = E.thresholds()
    assert thr[7] == 0.07 and 7 / 100 >= thr[7] and not 6 / 100 >= thr[7]
    assert E.k_min(100) == list(range(101)) and E.k_min(200)[7] == 14 and E.k_min(1)[1:] == [1] * 100 and E.k_min(3)[33:35] == [1, 2]
    for d in range(1, 1025):
        km = E.k_min(d)
        assert km[0] == 0 and km[100] == d
        for j in range(101):
            x = -(-j * d // 100)                            # the least x with 100 x >= j d
            assert km[j] == x and x / d >= thr[j] and (x == 0 or not (x - 1) / d >= thr[j]), (d, j)
    # a site at (100, 7): the draw of d = N = 100 is the site, 7 of 100 called -- 1 up to 0.07, 0 from 0.08
    diffs, positions = EC.build([('c', 5, '+', 'm6A', [1] * 7 + [0] * 93, None), ('c', 6, '+', 'A', [0] * 100, None)])
    t = E.evaluate_tables(diffs, positions, 1, (100,))[2]
    assert t['tpr'] == [1.0] * 8 + [0.0] * 93 and t['fpr'] == [1.0] + [0.0] * 100


def test_empty_classes_print_nan():
    from mcaller_amd import evaluate as E
    diffs, positions = EC.build([('c', 5, '+', 'm6A', [1, 0, 1], None), ('c', 9, '-', 'm', [1, 1], None)])
    out = E.evaluate_calls(diffs, positions, 2, (1, 3)).decode().split('\n')
    assert out[1] == 'read\t-\t0.0\t5\t0\t5\t0\t1.0\tnan' and out[1 + 101] == 'site\tall\t0.0\t2\t0\t2\t0\t1.0\tnan'
    assert out[-5:-1] == ['auc\tread\t-\tnan', 'auc\tsite\tall\tnan', 'auc\tsite\t1\tnan', 'auc\tsite\t3\tnan']
    # no row at all: both classes empty, every rate nan
    out = E.evaluate_calls(b'', positions, 2, (4,)).decode().split('\n')
    assert out[1] == 'read\t-\t0.0\t0\t0\t0\t0\tnan\tnan' and out[1 + 202] == 'site\t4\t0.0\t0\t0\t-\t-\tnan\tnan'
    assert E.last_eval['n_rows'] == 0 and E.last_eval['n_sites'] == 0


def test_depths_above_a_site_exclude_it_and_the_sites_own_depth_is_exact():
    from mcaller_amd import evaluate as E
    sites = [('c', 1, '+', 'm6A', [1, 1, 0, 1, 0], None), ('c', 2, '+', 'A', [0, 1, 0], None), ('c', 3, '+', 'm6A', [1], None)]
    diffs, positions = EC.build(sites)
    t1, t3, t5, t6 = E.evaluate_tables(diffs, positions, 1, (1, 3, 5, 6))[2:]
    assert (t1['n_pos'], t1['n_neg']) == (2, 1) and (t3['n_pos'], t3['n_neg']) == (1, 1)
    assert (t5['n_pos'], t5['n_neg']) == (1, 0) and (t6['n_pos'], t6['n_neg']) == (0, 0)
    assert all(math.isnan(v) for v in t6['tpr'] + t6['fpr']) and math.isnan(t5['auc'])
    # d == N: the draw is the site itself -- 3 of 5 called: 1 up to 0.6, 0 above
    assert t5['tpr'] == [1.0] * 61 + [0.0] * 40
    # d == N of the negative site (1 of 3 called): 1 up to 0.33, 0 from 0.34
    assert t3['fpr'] == [1.0] * 34 + [0.0] * 67
    # d == 1: K / N at every threshold above 0
    assert t1['fpr'][1:] == [1 / 3] * 100 and t1['tpr'][1:] == [float((Fraction(3, 5) + 1) / 2)] * 100 and t1['tpr'][0] == 1.0


def test_truth_rules_and_errors():
    from mcaller_amd import evaluate as E
    positions = b'c 5  +\tA\n\n \t \nc\t5\t+\tm6A\t\nc\t5\t+\tAm\textra\nd\t7\t-\tmm\nlonely\n'
    assert E.read_truth(positions) == {('c', 5, '+'): 'Am', ('d', 7, '-'): 'mm'}
    with pytest.raises(IndexError):
        E.read_truth(b'c\t5\t+\n')
    with pytest.raises(ValueError):
        E.read_truth(b'c\tx5\t+\tA\n')
    ok = EC.row('c', 5, '+', 'm6A', '0.5')
    assert E.evaluate_calls((ok + '\n').encode(), positions, 1, (1,)).decode().split('\n')[1] == 'read\t-\t0.0\t0\t1\t0\t1\tnan\t1.0'
    seven = '\t'.join(ok.split('\t')[:7])
    with pytest.raises(ValueError, match='line 2'):
        E.evaluate_calls((ok + '\n' + seven + '\n').encode(), positions, 1, (1,))
    with pytest.raises(ValueError, match='line 1'):
        E.evaluate_calls(b'\n', positions, 1, (1,))
    for prob in ('1.5', 'nan', '-0.1'):
        with pytest.raises(ValueError, match='outside'):
            E.evaluate_calls((EC.row('c', 5, '+', 'm6A', prob) + '\n').encode(), positions, 1, (1,))
    # an unlabelled row's probability is never looked at; ' 0.25 ' is stripped
    assert E.evaluate_calls((EC.row('c', 6, '+', 'm6A', 'junk') + '\n' + EC.row('d', 7, '-', 'A', ' 0.25 ') + '\n').encode(), positions, 1, (1,))
    assert (E.last_eval['n_unlabelled'], E.last_eval['n_kept'], E.last_eval['n_pos_sites']) == (1, 1, 1)
    for depths in ((0,), (1025,), (2, 2), (3, 2), tuple(range(1, 18))):
        with pytest.raises(ValueError, match='--depths'):
            E.evaluate_calls(b'', positions, 1, depths)
    assert E.evaluate_calls(b'', positions, 1, tuple(range(1, 17)))


def test_command_line_and_output_name(tmp_path, capsys, monkeypatch):
    """The default output is `<-f>.split('.')[0] + '.evaluation.tsv'`, make_bed's naming rule: the name is cut at the FIRST dot of the
    path as it was given, so the file is named from inside its directory here (a directory with a dot in its name cuts there)."""
    from mcaller_amd import evaluate as E
    diffs, positions = EC.random_case(6)
    monkeypatch.chdir(tmp_path)
    with open('reads.eventalign.diffs.6', 'wb') as fh:
        fh.write(diffs)
    with open('pos.txt', 'wb') as fh:
        fh.write(positions)
    out = E.main(['-f', 'reads.eventalign.diffs.6', '-p', 'pos.txt', '-d', '3', '--depths', '1,2,5'])
    assert out == 'reads.evaluation.tsv' == E.default_output('reads.eventalign.diffs.6')
    assert E.default_output('run.1/reads.diffs.6') == 'run.evaluation.tsv' and E.default_output('a/b.c.d') == 'a/b.evaluation.tsv'
    assert open(out, 'rb').read() == EC.brute_force(diffs, positions, 3, (1, 2, 5))[0]
    out = E.main(['-f', 'reads.eventalign.diffs.6', '-p', 'pos.txt', '-o', str(tmp_path / 'x.tsv')])
    assert out == str(tmp_path / 'x.tsv') and open(out, 'rb').read() == E.evaluate_calls(diffs, positions, 15, E.DEFAULT_DEPTHS)
    assert 'sites' in capsys.readouterr().err
    # the root shim runs the same main
    assert 'from mcaller_amd.evaluate import main' in open(os.path.join(H.REPO, 'evaluate.py')).read()


def test_the_references_test_data():
    """testdata/masonread1.eventalign.diffs.6 against test_positions.txt: nine rows, nine sites, every one labelled m6A (lines
    ending in a tab) -- no negative class, so every fpr and AUC is nan, and the rates are counts over nine."""
    from mcaller_amd import evaluate as E
    diffs, positions = os.path.join(TESTDATA, 'masonread1.eventalign.diffs.6'), os.path.join(TESTDATA, 'test_positions.txt')
    out = E.evaluate_calls(diffs, positions, 1, (1, 2))
    assert E.last_eval == dict(by='host', reason=None, n_rows=9, n_kept=9, n_unlabelled=0, n_not_m=0, n_sites=9, n_pos_sites=9, n_neg_sites=0)
    assert out == EC.brute_force(open(diffs, 'rb').read(), open(positions, 'rb').read(), 1, (1, 2))[0]
    lines = out.decode().split('\n')
    probs = [float(l.split('\t')[7]) for l in open(diffs).read().splitlines()]
    for j in (0, 10, 45, 50, 67, 71, 72, 100):
        n = sum(1 for p in probs if p >= j / 100)
        assert lines[1 + j] == 'read\t-\t%r\t9\t0\t%d\t0\t%s\tnan' % (j / 100, n, np.round(n / 9, 4))
    assert lines[1 + 303] == 'site\t2\t0.0\t0\t0\t-\t-\tnan\tnan' and lines[-4:-1] == ['auc\tsite\tall\tnan', 'auc\tsite\t1\tnan', 'auc\tsite\t2\tnan']
