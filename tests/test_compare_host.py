"""compare_genomes' host statement (compare_by_position: SciPy) on small hand-written --vo BED files: which keys get a row and in
which order, duplicate keys, lines that are not 8 fields, the same file twice, the command line.  Needs no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mcaller_amd import compare_genomes as CG
from tests import helpers as H
from tests import twosample_cases as T

A = [0.1, 0.2, 0.9, 0.35, 0.5]
B = [0.8, 0.7, 0.95, 0.4]
C = [0.3, 0.3, 0.6]


def write(tmp_path, name, lines):
    p = str(tmp_path / name)
    open(p, 'w').write(''.join(lines))
    return p


def rows(p1, p2):
    data, n = CG.compare_rows(p1, p2)
    out = [r.split('\t') for r in data.decode().splitlines()]
    assert len(out) == n and all(len(r) == 17 for r in out) and (not data or data.endswith(b'\n'))
    return out


def test_shared_keys_in_the_order_of_bed1(tmp_path):
    p1 = write(tmp_path, 'a', [T.bed_line('chr1', 30, '+', A), T.bed_line('chr1', 10, '-', B), T.bed_line('chr2', 10, '-', C),
                               T.bed_line('chr1', 20, '+', C)])
    p2 = write(tmp_path, 'b', [T.bed_line('chr1', 20, '+', A), T.bed_line('chr1', 10, '-', C), T.bed_line('chr3', 10, '-', C),
                               T.bed_line('chr1', 30, '+', B), T.bed_line('chr1', 10, '+', B)])
    out = rows(p1, p2)
    assert [tuple(r[:4]) for r in out] == [('chr1', '30', '31', '+'), ('chr1', '10', '11', '-'), ('chr1', '20', '21', '+')]
    first = out[0]
    assert first[4:8] == ['0.4', '5', '0.75', '4']                    # frac and depth of the two lines as they stand
    assert first[8:] == T.statement_text(A, B)
    assert first[8] == '4.0' and float(first[12]) == 3 / 5 - 0 / 4    # U of x (four pairs with x > y); D, at 0.35
    assert out[1][8:] == T.statement_text(B, C) and out[2][8:] == T.statement_text(C, A)


def test_sample_1_is_tested_against_sample_2(tmp_path):
    """Unlike the reference (compare_genomes.py:21-29), which tests bed1's sample against itself and prints nothing."""
    p1 = write(tmp_path, 'a', [T.bed_line('chr1', 30, '+', [0.1] * 10 + [0.2] * 10)])
    p2 = write(tmp_path, 'b', [T.bed_line('chr1', 30, '+', [0.8] * 10 + [0.9] * 10)])
    (r,) = rows(p1, p2)
    assert r[8] == '0.0' and r[12] == '1.0' and all(float(v) > 3.0 for v in r[13:])


def test_duplicate_keys_follow_the_dict_rule(tmp_path):
    """The first position, the last value."""
    p1 = write(tmp_path, 'a', [T.bed_line('chr1', 10, '+', A), T.bed_line('chr1', 20, '+', B), T.bed_line('chr1', 10, '+', C)])
    p2 = write(tmp_path, 'b', [T.bed_line('chr1', 20, '+', A), T.bed_line('chr1', 10, '+', B), T.bed_line('chr1', 20, '+', C)])
    out = rows(p1, p2)
    assert [r[1] for r in out] == ['10', '20']
    assert out[0][5] == '3' and out[0][8:] == T.statement_text(C, B)
    assert out[1][7] == '3' and out[1][8:] == T.statement_text(B, C)


@pytest.mark.parametrize('bad', ['chr1\t1\t2\tGATC\t0.5\t+\t0.1,0.2\n', 'chr1\t1\t2\tGATC\t0.5\t+\t2\t0.1,0.2\tx\ty\n', '\n'])
def test_a_line_that_is_not_8_fields_raises(tmp_path, bad):
    good = T.bed_line('chr1', 10, '+', A)
    for p1, p2 in ((write(tmp_path, 'a', [good, bad]), write(tmp_path, 'b', [good])),
                   (write(tmp_path, 'c', [good]), write(tmp_path, 'd', [bad, good]))):
        with pytest.raises(ValueError, match='unpack'):
            CG.compare_by_position(p1, p2, out=str(tmp_path / 'out'))


def test_a_number_float_rejects_raises(tmp_path):
    p1 = write(tmp_path, 'a', [T.bed_line('chr1', 10, '+', A).replace('0.35', '0.3x5')])
    with pytest.raises(ValueError, match='could not convert'):
        CG.compare_by_position(p1, p1, out=str(tmp_path / 'out'))


def test_the_same_file_twice(tmp_path):
    sites = T.depth_pairs(6, seed=3)
    t1, _, keys = T.bed_pair(sites)
    p = write(tmp_path, 'a', [t1.decode()])
    out = rows(p, p)
    assert [tuple(r[:4]) for r in out] == keys
    for r, (x, _) in zip(out, sites):
        assert r[8] == repr(len(x) * len(x) / 2) and r[12] == '0.0' and r[13:] == ['0.0'] * 4
        assert r[4:6] == r[6:8]


def test_last_compare_and_output_file(tmp_path):
    t1, t2, _ = T.bed_pair(T.depth_pairs(3, seed=4))
    p1, p2 = write(tmp_path, 'a', [t1.decode()]), write(tmp_path, 'b', [t2.decode()])
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position(p1, p2, None, out) == 3
    assert CG.last_compare['by'] == 'host' and CG.last_compare['n_sites'] == 3
    assert open(out, 'rb').read() == CG.compare_rows(p1, p2)[0]


def run(args, **kw):
    env = dict(os.environ, PYTHONPATH=H.REPO)
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, cwd=H.REPO, env=env, **kw)


def test_command_line(tmp_path):
    t1, t2, _ = T.bed_pair(T.depth_pairs(3, seed=4))
    p1, p2 = write(tmp_path, 'a', [t1.decode()]), write(tmp_path, 'b', [t2.decode()])
    want = CG.compare_rows(p1, p2)[0].decode()
    r = run(['-m', 'mcaller_amd.compare_genomes', '--bed1', p1, '--bed2', p2, '-g', 'unused.xmfa'])
    assert r.returncode == 0 and r.stdout == want, r.stderr
    out = str(tmp_path / 'out.tsv')
    r = run([os.path.join(H.REPO, 'compare_genomes.py'), '--bed1', p1, '--bed2', p2, '-o', out])
    assert r.returncode == 0 and r.stdout == '' and open(out).read() == want, r.stderr
    r = run(['-m', 'mcaller_amd.compare_genomes', '-v'])
    assert r.returncode == 0 and r.stdout == 'mCallerNP 0.3\n'
    r = run(['-m', 'mcaller_amd.compare_genomes', '--bed1', p1])
    assert r.returncode == 2 and '--bed2' in r.stderr
    r = run(['-m', 'mcaller_amd.compare_genomes', '--bed1', p1, '--bed2', str(tmp_path / 'missing')])
    assert r.returncode != 0 and 'file not found' in r.stderr
    r = run(['-m', 'mcaller_amd.compare_genomes', '--help'])
    assert 'bed file 1 with verbose output from make_bed.py' in r.stdout and 'an xmfa file from mauve' in r.stdout
