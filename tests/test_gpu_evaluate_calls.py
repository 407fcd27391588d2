"""`evaluate --device` (csrc/eval/mc_evalcalls.hip): the evaluation file made on the GPU is the host statement's, byte for byte,
or the call declines and says why.  "device == host" below always means both: the bytes are evaluate_calls' (for the small
random cases: the brute force's) AND last_eval['by'] == 'device' -- a silent decline does not pass as success."""
import os

import numpy as np
import pytest

from tests import evaluate_cases as EC
from tests import helpers as H

pytestmark = pytest.mark.gpu

TESTDATA = os.path.join(H.GOLDEN, 'testdata')
PAIRS = ((3, (1, 2, 3, 5, 10)), (1, (1, 4, 7, 9)), (11, (2,)))


def E():
    from mcaller_amd import evaluate
    return evaluate


def served(diffs, positions, min_depth, depths, want=None):
    """device == host -> the bytes."""
    if want is None:
        want = E().evaluate_calls(diffs, positions, min_depth, depths)
        host = dict(E().last_eval)
    else:
        host = None
    got = E().evaluate_calls_device(diffs, positions, min_depth, depths)
    assert got is not None, E().last_eval['reason']
    assert E().last_eval['by'] == 'device' and E().last_eval['reason'] is None
    assert got == want, [(a, b) for a, b in zip(got.split(b'\n'), want.split(b'\n')) if a != b][:5]
    if host is not None:                                     # the counters too
        assert dict(E().last_eval, by='host') == host
    return got


def declined(diffs, positions, min_depth, depths, reason, line=None, file=0):
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    assert E().evaluate_calls_device(diffs, positions, min_depth, depths) is None
    s = get_device().eval_calls_last_stats()
    assert s['decline_reason'] == _lib.EVAL_DECLINE[reason], (s, E().last_eval['reason'])
    assert s['decline_file'] == file
    if line is not None:
        assert s['decline_line'] == line and 'line %d' % (line + 1) in E().last_eval['reason']
    return E().last_eval['reason']


def tie_free(diffs, positions, min_depth, depths):
    """No expected-table value within 1e-9 of a tie of np.round(., 4) -- decided on exact rationals.  1e-9 is a thousand times the
    largest bound a value can carry (below 1e-12: profiles/hypergeom_error.json, and the finishing operations add 3e-14), so a case
    that is tie-free in this sense may not be declined.  (Seeds 7, 10 and 102 have a value 8e-7 from a tie: a margin of 1e-6 would
    not hold for them, and is not needed.)"""
    from fractions import Fraction
    for t in E().evaluate_tables(diffs, positions, min_depth, depths)[2:]:
        for v in t['exact']:
            if v is not None:
                frac = v * 10000 - (v * 10000).__floor__()
                if abs(frac - Fraction(1, 2)) <= Fraction(1, 100000):
                    return False
    return True


@pytest.mark.parametrize('on_grid', [True, False])
@pytest.mark.parametrize('seed', [6, 7, 8, 10, 11, 13])
def test_small_random_cases_are_the_brute_force(seed, on_grid):
    diffs, positions = EC.random_case(seed, on_grid=on_grid)
    for min_depth, depths in PAIRS:
        assert tie_free(diffs, positions, min_depth, depths)                   # so the device may not decline
        want, _ = EC.brute_force(diffs, positions, min_depth, depths)
        served(diffs, positions, min_depth, depths, want)
    assert (E().last_eval['n_unlabelled'], E().last_eval['n_not_m'], E().last_eval['n_sites']) == (6, 2, 14)


@pytest.mark.parametrize('seed', [101, 102, 103])
def test_larger_random_cases_are_the_host_statement(seed):
    diffs, positions = EC.random_case(seed, n_sites=300, max_n=60)
    assert tie_free(diffs, positions, 15, E().DEFAULT_DEPTHS)
    served(diffs, positions, 15, E().DEFAULT_DEPTHS)


@pytest.mark.parametrize('seed', [12, 16])
def test_tie_seeds_give_the_hosts_bytes_or_decline(seed, tmp_path):
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    diffs, positions = EC.random_case(seed)
    min_depth, depths = PAIRS[0]
    assert not tie_free(diffs, positions, min_depth, depths)
    want = E().evaluate_calls(diffs, positions, min_depth, depths)
    got = E().evaluate_calls_device(diffs, positions, min_depth, depths)
    if got is None:
        assert get_device().eval_calls_last_stats()['decline_reason'] == _lib.EVAL_DECLINE['rounding_tie']
    else:
        assert got == want and E().last_eval['by'] == 'device'
    (tmp_path / 'a.diffs.6').write_bytes(diffs)
    (tmp_path / 'p.txt').write_bytes(positions)
    out = E().main(['--device', '-f', str(tmp_path / 'a.diffs.6'), '-p', str(tmp_path / 'p.txt'), '-d', str(min_depth), '--depths',
                    ','.join(str(d) for d in depths), '-o', str(tmp_path / 'out.tsv')])
    assert open(out, 'rb').read() == want
    assert (E().last_eval['by'], E().last_eval['reason'] is None) == (('device', True) if got is not None else ('host', False))


def test_a_constructed_tie_declines_and_its_trivial_twin_is_served():
    """1/32 = 0.03125 from two tails of 1/2: on a tie of four decimals, and the device cannot know which side the exact value is on."""
    sites = [('c', 10 + i, '+', 'm6A', [1, 0] if i < 2 else [0, 0], None) for i in range(32)] + [('c', 900, '+', 'A', [0, 0], None)]
    diffs, positions = EC.build(sites, shuffle_seed=1)
    declined(diffs, positions, 1, (1,), 'rounding_tie')
    got = served(diffs, positions, 1, (2,))                                    # d = N: every mass trivial, bound 0
    from mcaller_amd.device import get_device
    assert get_device().eval_calls_last_stats()['largest_bound'] == 0.0
    assert b"site\t2\t0.01\t32\t1\t-\t-\t0.0625\t0.0\n" in got


@pytest.mark.parametrize('n', [255, 256, 257])
def test_the_staged_tile_edges(n):
    """n .diffs lines and n positions lines: the last workgroup of ke_rows holds 255, 256 or 1 line."""
    rng = np.random.RandomState(n)
    sites = [('c%d' % (i % 3), 10 + i, '+-'[i % 2], 'm6A' if i % 3 else 'A', [int(rng.rand() < 0.5)], None) for i in range(n)]
    diffs, positions = EC.build(sites, shuffle_seed=n)
    assert diffs.count(b'\n') == n and positions.count(b'\n') == n
    served(diffs, positions, 1, (1, 2))
    served(diffs[:-1], positions[:-1], 1, (1,))                                # no newline behind the last line of either


def test_empty_files_empty_classes_and_the_references_test_data():
    diffs, positions = EC.build([('c', 5, '+', 'm6A', [1, 0, 1], None), ('c', 9, '-', 'm', [1, 1], None)])
    out = served(diffs, positions, 2, (1, 3)).decode().split('\n')
    assert out[1] == 'read\t-\t0.0\t5\t0\t5\t0\t1.0\tnan' and out[-5:-1] == ['auc\tread\t-\tnan', 'auc\tsite\tall\tnan', 'auc\tsite\t1\tnan', 'auc\tsite\t3\tnan']
    out = served(b'', positions, 2, (4,)).decode().split('\n')
    assert out[1] == 'read\t-\t0.0\t0\t0\t0\t0\tnan\tnan' and out[1 + 202] == 'site\t4\t0.0\t0\t0\t-\t-\tnan\tnan'
    served(diffs, b'', 2, (1,))
    served(b'', b'', 2, ())
    d, p = os.path.join(TESTDATA, 'masonread1.eventalign.diffs.6'), os.path.join(TESTDATA, 'test_positions.txt')
    served(d, p, 1, (1, 2))
    assert E().last_eval == dict(by='device', reason=None, n_rows=9, n_kept=9, n_unlabelled=0, n_not_m=0, n_sites=9, n_pos_sites=9, n_neg_sites=0)
    served(open(d, 'rb').read(), open(p, 'rb').read(), 1, (1, 2))             # paths and texts: the same bytes


def test_a_site_whose_rows_sit_in_different_workgroups():
    calls = [1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 1]
    filler = [EC.row('other', 7000 + i, '+', 'A', '0.4') for i in range(700)]
    rows = EC.site_rows('c', 5, '+', calls) + EC.site_rows('c', 6, '-', [0, 0, 1, 0, 0, 0, 1, 0], probs=['0.07'] * 8)
    mixed = []
    for i, r in enumerate(rows):                                               # a row of the two sites every 35 lines
        mixed += filler[35 * i:35 * (i + 1)] + [r]
    diffs = ('\n'.join(mixed) + '\n').encode()
    positions = b'c\t5\t+\tm6A\nc\t6\t-\tA\nother\t7003\t+\tA\n'
    served(diffs, positions, 5, (1, 3, 8, 12))
    assert (E().last_eval['n_sites'], E().last_eval['n_kept'], E().last_eval['n_unlabelled']) == (3, 21, 699)


def test_the_truth_rules():
    ok = EC.row('c', 5, '+', 'm6A', '0.5') + '\n' + EC.row('d', 7, '-', 'A', '0.25') + '\n' + EC.row('c', 7, '+', 'A', '0.75') + '\n'
    # a key twice with different labels (the last wins), blanks and tabs mixed, a trailing tab, 007 for 7, a one-token line
    positions = b'c 5  +\tA\n\n \t \nc\t5\t+\tm6A\t\nc\t5\t+\tAm\textra\nd\t007\t-\tmm\nlonely\nc\t7\t+ m\t\n'
    out = served(ok.encode(), positions, 1, (1,)).decode().split('\n')
    assert out[1] == 'read\t-\t0.0\t2\t1\t2\t1\t1.0\t1.0' and E().last_eval['n_pos_sites'] == 2
    declined(ok.encode(), positions + b'c\t5\t+\n', 1, (1,), 'pos_tokens', line=8, file=1)         # the host's IndexError
    declined(ok.encode(), b'c\tx5\t+\tA\n', 1, (1,), 'pos_number', line=0, file=1)
    declined(ok.encode(), b'c\t+5\t+\tA\n', 1, (1,), 'pos_number', line=0, file=1)                  # int() takes it; the device does not guess
    declined(ok.encode(), b'c\t5\t+\tA\r\n', 1, (1,), 'control', line=0, file=1)
    declined(ok.encode(), 'c\t5\t+\té\n'.encode('utf-8'), 1, (1,), 'high_byte', line=0, file=1)


def test_the_row_rules():
    positions = b'c\t5\t+\tm6A\nd\t7\t-\tA\n'
    good = [EC.row('c', 5, '+', 'm6A', '0.5'), EC.row('d', 7, '-', 'A', ' 0.25 ')]
    skipped = [EC.row('c', 'junk', '+', 'A', '0.3', EC.CONTEXT_A),             # no centre M: the position is never read
               EC.row('c', 6, '+', 'm6A', 'junk')]                             # unlabelled: the probability is never read
    served(('\n'.join(good + skipped) + '\n').encode(), positions, 1, (1,))
    assert (E().last_eval['n_not_m'], E().last_eval['n_unlabelled'], E().last_eval['n_kept']) == (1, 1, 2)
    for prob in ('1.5', 'nan', 'junk', '-0.1', ''):
        declined(('\n'.join(good + [EC.row('c', 5, '+', 'A', prob)]) + '\n').encode(), positions, 1, (1,), 'probability', line=2)
    seven = '\t'.join(good[0].split('\t')[:7])
    declined(('\n'.join(good + skipped + [seven] + good) + '\n').encode(), positions, 1, (1,), 'fields', line=4)
    declined(('\n'.join(good) + '\n\n').encode(), positions, 1, (1,), 'fields', line=2)             # an empty line
    declined((good[0] + '\n' + EC.row('c', 'x', '+', 'A', '0.3') + '\n').encode(), positions, 1, (1,), 'position', line=1)
    declined((EC.row('c', 5, '+', 'A', '0.3', context='') + '\n').encode(), positions, 1, (1,), 'context', line=0)
    declined((good[0] + '\r\n').encode(), positions, 1, (1,), 'control', line=0)


def test_the_knobs(monkeypatch, tmp_path):
    diffs, positions = EC.random_case(7, n_sites=40)
    want = E().evaluate_calls(diffs, positions, 3, (1, 2, 5))
    monkeypatch.setenv('MCALLER_EVAL_HASH_MASK', 'f')                          # every key in one of 16 chains
    served(diffs, positions, 3, (1, 2, 5), want)
    from mcaller_amd.device import get_device
    assert get_device().eval_calls_last_stats()['longest_probe'] >= 2
    monkeypatch.delenv('MCALLER_EVAL_HASH_MASK')
    monkeypatch.setenv('MCALLER_EVAL_TABLE_SLOTS', '8')
    declined(diffs, positions, 3, (1, 2, 5), 'table', file=1)
    monkeypatch.delenv('MCALLER_EVAL_TABLE_SLOTS')
    monkeypatch.setenv('MCALLER_EVAL_DEVICE_BYTES', '1000')
    declined(diffs, positions, 3, (1, 2, 5), 'memory')
    monkeypatch.delenv('MCALLER_EVAL_DEVICE_BYTES')
    (tmp_path / 'a.diffs.6').write_bytes(diffs)
    (tmp_path / 'p.txt').write_bytes(positions)
    monkeypatch.setenv('MCALLER_TEXT_STAGE_BYTES', '256')                      # the files in blocks of 256 bytes
    served(str(tmp_path / 'a.diffs.6'), str(tmp_path / 'p.txt'), 3, (1, 2, 5), want)


def test_the_depths():
    # d = N, K = 0, K = N; one draw; a depth above every site
    sites = [('c', 1, '+', 'm6A', [1, 1, 0, 1, 0], None), ('c', 2, '+', 'A', [0, 1, 0], None), ('c', 3, '+', 'm6A', [1], None),
             ('c', 4, '+', 'A', [0] * 7, None), ('c', 5, '+', 'm6A', [1] * 6, None)]
    diffs, positions = EC.build(sites)
    served(diffs, positions, 1, (3, 5, 6, 7))
    out = served(diffs, positions, 1, (1, 8)).decode().split('\n')
    assert out[1 + 303] == 'site\t8\t0.0\t0\t0\t-\t-\tnan\tnan' and out[-2] == 'auc\tsite\t8\tnan'
    # deep sites: d = 1, 2, 1024 at N = 1024, 1025, 2000 -- a walk of a thousand steps, a stop below 2^-900
    rng = np.random.RandomState(3)
    deep = [('big', 10 * i, '+', 'm6A' if i % 2 else 'A', list((rng.rand(n) < (0.7 if i % 2 else 0.45)).astype(int)), None)
            for i, n in enumerate((1024, 1025, 2000, 1024, 2000))]
    diffs, positions = EC.build(deep)
    assert tie_free(diffs, positions, 15, (1, 2, 1024))
    served(diffs, positions, 15, (1, 2, 1024))
    # 16 depths at once
    diffs, positions = EC.random_case(21, n_sites=60, max_n=40)
    depths = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 20, 25, 30, 40)
    if tie_free(diffs, positions, 15, depths):
        served(diffs, positions, 15, depths)
    else:
        want = E().evaluate_calls(diffs, positions, 15, depths)
        assert E().evaluate_calls_device(diffs, positions, 15, depths) in (None, want)


def test_three_runs_give_the_same_bytes_and_the_same_bound():
    from mcaller_amd.device import get_device
    diffs, positions = EC.random_case(102, n_sites=300, max_n=60)
    runs = []
    for _ in range(3):
        data = E().evaluate_calls_device(diffs, positions, 15, E().DEFAULT_DEPTHS)
        s = get_device().eval_calls_last_stats()
        runs.append((data, s['largest_bound'], s['n_expect'], s['n_sites']))
    assert runs[0][0] is not None and runs[0] == runs[1] == runs[2] and 0.0 < runs[0][1] < 1e-12


def test_device_masses_against_exact_rationals_and_the_host_build():
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    from tests import test_hypergeom_masses as M
    N, K, d = M.shapes()
    mass, err = get_device().hypergeom_masses(N, K, d)                         # one launch
    worst = M.check_masses(N, K, d, mass, err, M.k_min)
    assert 0.0 < worst < 2e-12
    h_mass, h_err = _lib.hypergeom_masses(N, K, d)
    assert (np.abs(mass - h_mass).sum(axis=1) <= err + h_err).all()
    exact = h_err == 0.0
    assert exact.any() and (mass[exact] == h_mass[exact]).all() and (err[exact] == 0.0).all()
    bad, _ = get_device().hypergeom_masses([5], [6], [1])
    assert np.isnan(bad).all() and get_device().hypergeom_masses([], [], [])[0].shape == (0, 102)
