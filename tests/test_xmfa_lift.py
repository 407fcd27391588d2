"""compare_genomes through a Mauve alignment, the host statement (compare_genomes.xmfa_map, lift_key, compare_rows(xmfa_path=)):
against tests/xmfa_cases.py's brute force over the columns on seeded random alignments, on the identity alignment, on a base aligned
twice, on a three-genome file; every error of the definition with its line; the command line.  Needs no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mcaller_amd import compare_genomes as CG
from tests import helpers as H
from tests import xmfa_cases as X

RANDOM = X.random_cases(200)


def lift_of(P, c):
    return dict(xmfa_path=P['xmfa'], fai1=P['fai1'], fai2=P['fai2'], seqs=c['seqs'])


def test_the_generator_covers_what_it_says():
    texts = b''.join(c['xmfa'] for c in RANDOM).decode()
    assert {c['seqs'] for c in RANDOM} == {(1, 2), (3, 1)}
    assert ':0-0 ' in texts and '> 3:' in texts
    flips = set()
    for c in RANDOM:
        assert c['n_rows'] >= 1 and len(c['mapping']) >= 1
        flips |= {f for _, f in c['mapping'].values()}
        assert 'ghost' in c['bed1'].decode()                           # (a line without an image; beds() asserts both kinds)
    assert flips == {0, 1}
    assert any(len(c['mapping']) < c['n1'] for c in RANDOM)
    assert any(('> %d:' % c['seqs'][1]) not in block for c in RANDOM for block in c['xmfa'].decode().split('\n=\n')[:-1])


def test_the_edges_hold_what_they_are_named_for():
    sets = X.edge_block_sets()
    assert [len(e[0][4]) for e in sets['block sizes'][1]] == [1, 63, 64, 65, 129]
    assert sorted({e[5] for b in sets['line widths'][1] for e in b}) == [1, 63, 64, 65, 80]
    t1 = sets['gaps at word edges'][1][0][0][4]
    assert t1[60:70] == '-' * 10 and t1[59] != '-' and t1[70] != '-'                      # a run over column 64
    (a, b), = sets['first and last column a gap'][1]
    assert a[4][0] == '-' and b[4][-1] == '-'
    lens, blocks, want = sets['contig edges']
    assert blocks[0][0][1] == 1 and blocks[0][0][2] == sum(lens[1]) and {1, 40, 41, 100, 50, 51} <= set(want)
    assert len(sets['257 entries'][1][0]) == 257 and X.edge_case('257 entries')['xmfa'].count(b'\n') > 2 * 256


def test_the_map_equals_the_brute_force(tmp_path):
    for c in RANDOM:
        P = X.write(tmp_path, c)
        g2, flip = CG.xmfa_map(P['xmfa'], c['n1'], c['seqs'], c['n2'])
        want_g2, want_flip = X.brute_arrays(c['xmfa'], c['n1'], c['seqs'])
        assert g2.dtype == np.int64 and flip.dtype == np.uint8 and len(g2) == len(flip) == c['n1'] + 1
        assert np.array_equal(g2, want_g2) and np.array_equal(flip, want_flip), c['name']


def test_the_rows_equal_the_brute_force_lift(tmp_path):
    for c in RANDOM[:30] + X.edge_cases() + [X.unpaired_case()]:
        P = X.write(tmp_path, c)
        want, n, n_unaligned = X.expected_rows(c)
        assert CG.compare_rows(P['bed1'], P['bed2'], **lift_of(P, c)) == (want, n), c['name']
        assert n >= c['n_rows'] and n_unaligned >= 1 and all(len(r.split('\t')) == 21 for r in want.decode().splitlines())
        out = str(tmp_path / 'out.tsv')
        assert CG.compare_by_position(P['bed1'], P['bed2'], None, out, **lift_of(P, c)) == n
        assert CG.last_compare == dict(by='host', reason='the host statement was asked for', n_sites=n, n_unaligned=n_unaligned)
        assert open(out, 'rb').read() == want


def test_the_identity_alignment_repeats_the_key(tmp_path):
    c = X.identity_case()
    P = X.write(tmp_path, c)
    for bed in ('bed1', 'bed2'):                                       # (without the lines on a contig no .fai knows)
        open(P[bed], 'wb').write(b''.join(line for line in c[bed].splitlines(True) if not line.startswith(b'ghost')))
    base, n = CG.compare_rows(P['bed1'], P['bed2'])
    assert n >= 2
    want = ''.join('\t'.join(r.split('\t')[:4] + r.split('\t')) + '\n' for r in base.decode().splitlines()).encode()
    assert CG.compare_rows(P['bed1'], P['bed2'], **lift_of(P, c)) == (want, n)


def test_the_first_column_of_a_base_wins(tmp_path):
    t = X.letters(10)
    blocks = [[(1, 1, 10, '+', t, 80), (2, 21, 30, '-', t, 80)], [(1, 6, 15, '+', t, 80), (2, 1, 10, '+', t, 80)]]
    p = str(tmp_path / 'twice.xmfa')
    open(p, 'wb').write(X.xmfa_text(blocks))
    g2, flip = CG.xmfa_map(p, 15, (1, 2), 30)
    assert g2.tolist() == [0] + list(range(30, 20, -1)) + [6, 7, 8, 9, 10]
    assert flip.tolist() == [0] + [1] * 10 + [0] * 5
    assert (g2 == X.brute_arrays(X.xmfa_text(blocks), 15)[0]).all()


def test_other_sequence_numbers_of_a_three_genome_file(tmp_path):
    a, b, c3 = X.letters(6), 'AC--GTAC', 'ACGTAC--'
    blocks = [[(1, 3, 8, '+', a + '--', 7), (2, 1, 6, '+', b, 1), (3, 5, 10, '-', c3, 64)]]
    p = str(tmp_path / 'three.xmfa')
    open(p, 'wb').write(X.xmfa_text(blocks))
    g2, flip = CG.xmfa_map(p, 10, (3, 1), 8)
    assert g2.tolist() == [0, 0, 0, 0, 0, 8, 7, 6, 5, 4, 3] and flip[5:].tolist() == [1] * 6
    g2, flip = CG.xmfa_map(p, 6, (2, 3))
    assert g2.tolist() == [0, 10, 9, 6, 5, 0, 0]
    with pytest.raises(ValueError, match='two different'):
        CG.xmfa_map(p, 6, (2, 2))


BAD = X.bad_xmfas()


@pytest.mark.parametrize('name', sorted(BAD))
def test_every_error_names_its_line(tmp_path, name):
    text, _, line = BAD[name]
    p = str(tmp_path / 'bad.xmfa')
    open(p, 'wb').write(text)
    with pytest.raises(ValueError, match=r'^xmfa line %d: ' % (line + 1)):
        CG.xmfa_map(p, 8, (1, 2), 8)


def test_the_good_file_of_the_error_cases_is_good(tmp_path):
    p = str(tmp_path / 'good.xmfa')
    open(p, 'w').write('\n'.join(X.GOOD) + '\n')
    assert CG.xmfa_map(p, 8, (1, 2), 8)[0].tolist() == [0, 8, 7, 6, 5, 4, 3, 2, 1]


def test_a_start_int_takes_is_lifted_and_one_it_rejects_has_no_image(tmp_path):
    c = X.identity_case()
    P = X.write(tmp_path, c)
    lines = c['bed1'].decode().splitlines(True)
    first = lines[0].split('\t')
    odd = ['\t'.join([first[0], form] + first[2:]) for form in ('+7', '007', '1_0', 'x', '-1')]
    open(P['bed1'], 'w').write(''.join(odd))
    open(P['bed2'], 'w').write(''.join('\t'.join([first[0], s, str(int(s) + 1)] + first[3:]) for s in ('7', '10')))
    data, n = CG.compare_rows(P['bed1'], P['bed2'], **lift_of(P, c))
    assert [r.split('\t')[1] + '>' + r.split('\t')[5] for r in data.decode().splitlines()] == ['+7>7', '007>7', '1_0>10'] and n == 3
    CG.compare_by_position(P['bed1'], P['bed2'], out=str(tmp_path / 'o'), **lift_of(P, c))
    assert CG.last_compare['n_unaligned'] == 2


def test_read_fai(tmp_path):
    p = str(tmp_path / 'g.fai')
    open(p, 'w').write('chrA\t10\t6\t60\t61\n\nchrB\t0\nchrA\t5\t99\n')
    names, lens, offs = CG.read_fai(p)
    assert names == ['chrA', 'chrB', 'chrA'] and lens.tolist() == [10, 0, 5] and offs.tolist() == [0, 10, 10, 15]
    open(p, 'w').write('chrA\tten\n')
    with pytest.raises(ValueError, match='line 1'):
        CG.read_fai(p)


def run(args):
    env = dict(os.environ, PYTHONPATH=H.REPO)
    return subprocess.run([sys.executable, '-m', 'mcaller_amd.compare_genomes'] + args, capture_output=True, text=True, cwd=H.REPO, env=env)


def test_command_line(tmp_path, capfd):
    c = RANDOM[0]
    P = X.write(tmp_path, c)
    want, n, n_unaligned = X.expected_rows(c)
    beds = ['--bed1', P['bed1'], '--bed2', P['bed2']]
    r = run(beds + ['--xmfa', P['xmfa'], '--fai2', P['fai2']])
    assert r.returncode == 2 and '--fai1' in r.stderr
    r = run(beds + ['--xmfa', P['xmfa'], '--fai1', P['fai1'], '--fai2', P['fai2'], '--xmfa_seqs', '1,1'])
    assert r.returncode == 2 and 'xmfa_seqs' in r.stderr
    seqs = ['--xmfa_seqs', '%d,%d' % c['seqs']]
    r = run(beds + ['-g', str(tmp_path / 'nonexistent.xmfa'), '--xmfa', P['xmfa'], '--fai1', P['fai1'], '--fai2', P['fai2']] + seqs)
    assert r.returncode == 0 and r.stdout.encode() == want, r.stderr
    out = str(tmp_path / 'out.tsv')
    CG.main(beds + ['--xmfa', P['xmfa'], '--fai1', P['fai1'], '--fai2', P['fai2'], '-o', out] + seqs)
    assert capfd.readouterr().out == '' and open(out, 'rb').read() == want
    assert CG.last_compare['n_unaligned'] == n_unaligned and CG.last_compare['n_sites'] == n
    r = run(beds + ['-g', str(tmp_path / 'nonexistent.xmfa')])
    assert r.returncode == 0 and r.stdout.encode() == CG.compare_rows(P['bed1'], P['bed2'])[0]
    assert 'n_unaligned' not in (CG.compare_by_position(P['bed1'], P['bed2'], out=out), CG.last_compare)[1]
