"""find_motifs' host statement (mcaller_amd/find_motifs.py, NumPy) against the brute-force restatement of tests/motif_sites.py, the
placed cases, selection and redundancy edges, the order, every ValueError, the planted-motif condition and the command line.
Needs no GPU."""
import os
import subprocess
import sys

import pytest

from mcaller_amd import find_motifs as FM
from mcaller_amd import refmark
from tests import helpers as H
from tests import motif_sites as MS


def files(tmp_path, contigs, bed, control=None, form='plain'):
    ref, pb = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed')
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(MS.bed_text(bed, form))
    pc = None
    if control is not None:
        pc = str(tmp_path / 'control.bed')
        open(pc, 'wb').write(MS.bed_text(control))
    return ref, pb, pc


def run(tmp_path, contigs, bed, control=None, **kw):
    ref, pb, pc = files(tmp_path, contigs, bed, control)
    out = str(tmp_path / 'out.tsv')
    n = FM.find_motifs(ref, pb, pc, out=out, **kw)
    data = open(out, 'rb').read()
    assert n == data.count(b'\n') and FM.last_report == dict(by='host', reason='the host statement was asked for', n_rows=n)
    return data


def specs(data):
    return [line.split('\t')[0] for line in data.decode().splitlines()]


@pytest.mark.parametrize('seed,lengths,base,with_control,shapes', [
    (1, [1200, 300], 'A', True, None),
    (2, [300, 700, 450], 'A', False, None),
    (3, [900, 600], 'C', True, None),
    (4, [1500, 333], 'A', True, ['XX', 'X.X', 'X..X..X..X..X..X..X....X', 'XXXX']),
    (5, [800, 801], 'C', False, ['XX', 'X.X', 'X..X..X..X..X..X..X....X']),
])
def test_host_statement_equals_brute_force(tmp_path, seed, lengths, base, with_control, shapes):
    motif, called = ('GATC', 1) if base == 'A' else ('GCAGT', 1)
    contigs, bed, control = MS.random_case(seed, lengths, base, motif, called, with_control)
    shapes = MS.default_shapes() if shapes is None else shapes
    assert len(shapes[-2 if len(shapes) == 4 else -1]) <= 24
    tables = MS.brute_tables(contigs, bed, control, base, shapes)
    for kw in (dict(min_sites=3, min_fraction=0.5), dict(min_sites=1, min_fraction=0.0, keep_all=True)):
        got = run(tmp_path, contigs, bed, control, base=base, shapes=shapes, **kw)
        want = MS.brute(contigs, bed, control, base, shapes, tables=tables, **kw)
        assert got == want
    assert got.count(b'\n') >= 10


def test_default_shapes_are_those_of_the_definition():
    assert FM.DEFAULT_SHAPES == MS.default_shapes() and len(FM.DEFAULT_SHAPES) == 20
    assert sum(s.count('X') for s in FM.DEFAULT_SHAPES) == 130


def test_placed_cases(tmp_path):
    contigs, bed, control, shapes = MS.placed_case()
    for kw in (dict(min_sites=1, min_fraction=0.0, keep_all=True), dict(min_sites=2, min_fraction=0.3), dict(min_sites=0, min_fraction=0.0, keep_all=True)):
        for ctl in (control, None):
            got = run(tmp_path, contigs, bed, ctl, shapes=shapes, **kw)
            assert got == MS.brute(contigs, bed, ctl, 'A', shapes, **kw) and got
    run(tmp_path, contigs, bed, control, shapes=shapes)
    c = FM.last_counts
    n_cand = len(MS.candidates(contigs, 'A'))
    assert c['n_candidates'] == n_cand and c['n_sites'] == len(set(bed)) and c['n_control'] == len(set(control))
    assert c['n_off_base'] == 4                      # left:1+, right:1-, left:11+ (an N) and poly:0+ of the control


def test_letters_under_x_and_under_dot(tmp_path):
    """N, a lower-case letter and an IUPAC letter: not counted under an X, counted under a '.'; lower case is upper-cased."""
    contigs = [('c', 'CANGC' 'CARGC' 'CAgGC' 'CACGC')]
    bed = [('c', 1, '+'), ('c', 6, '+'), ('c', 11, '+'), ('c', 16, '+')]
    rows = {r.split('\t')[0]: r.split('\t')[1:] for r in run(tmp_path, contigs, bed, shapes=['X.X', 'XXX'], min_sites=1, keep_all=True).decode().splitlines()}
    assert rows['ANG:1'][:3] == ['4', '4', '4']      # the free letter is N, R, g, C
    assert rows['CAG:2'][:3] == ['1', '1', '1'] and rows['CAC:2'][:3] == ['1', '1', '1']
    assert not any(s.startswith(('CAN', 'CAR')) for s in rows)


def test_window_ends_and_short_contigs(tmp_path):
    contigs = [('a', 'ACCA'), ('b', 'A'), ('e', ''), ('t', 'TGGT')]
    bed = [('a', 0, '+'), ('a', 3, '+'), ('b', 0, '+'), ('t', 0, '-'), ('t', 3, '-')]
    got = run(tmp_path, contigs, bed, shapes=['XX', 'X..X'], min_sites=1, keep_all=True)
    assert got == MS.brute(contigs, bed, None, 'A', ['XX', 'X..X'], 1, 0.5, True)
    rows = {r.split('\t')[0]: int(r.split('\t')[3]) for r in got.decode().splitlines()}
    # 'a': AC at 0 (j = 0), CA at 3 (j = 1), ACCA both ways; 't' on '-': revcomp(TGGT) = ACCA, the same windows again
    assert rows == {'AC:1': 2, 'CA:2': 2, 'ANNA:1': 2, 'ANNA:4': 2}


def test_motif_methylated_on_one_strand_only(tmp_path):
    """GAAC (not its own reverse complement) methylated at its second A wherever it stands on '+': its row is there; no row
    is selected from the '-' occurrences, which are the GTTC of '+' and are not listed."""
    contigs = MS.random_genome(7, [4000])
    seq = contigs[0][1]
    bed = [('ctg0', p + 2, '+') for p in range(len(seq) - 3) if seq[p:p + 4] == 'GAAC']
    n_minus = sum(1 for p in range(len(seq) - 3) if seq[p:p + 4] == 'GTTC')
    assert len(bed) >= 5 and n_minus >= 5
    rows = {r.split('\t')[0]: r.split('\t')[1:] for r in run(tmp_path, contigs, bed, shapes=['XXXX'], min_sites=5, min_fraction=0.4).decode().splitlines()}
    n = len(bed)
    assert rows == {'GAAC:3': [str(n + n_minus), str(n + n_minus), str(n), repr(n / (n + n_minus))]} or n / (n + n_minus) < 0.4
    only_plus = [('ctg0', p, '-') for p in range(len(seq)) if seq[p] == 'T']
    rows = specs(run(tmp_path, contigs, bed, only_plus[:0] or None, shapes=['XXXX'], min_sites=1, min_fraction=0.0, keep_all=True))
    assert 'GAAC:3' in rows and 'GTTC:3' not in rows and 'GAAC:2' not in rows


def ten_of_twenty():
    """Twenty CAG on '+' (and no A elsewhere on either strand), ten of them listed."""
    seq = 'CCAGC' * 20
    return [('c', seq)], [('c', 5 * i + 2, '+') for i in range(10)]


def test_min_fraction_met_exactly_and_min_sites_edge(tmp_path):
    contigs, bed = ten_of_twenty()
    assert specs(run(tmp_path, contigs, bed, shapes=['XXX'], min_sites=10, min_fraction=0.5)) == ['AGC:1', 'CAG:2', 'CCA:3']
    assert specs(run(tmp_path, contigs, bed, shapes=['XXX'], min_sites=11, min_fraction=0.5)) == []
    assert specs(run(tmp_path, contigs, bed, shapes=['XXX'], min_sites=10, min_fraction=0.5000001)) == []
    assert run(tmp_path, contigs, bed, shapes=['X.X'], min_sites=10) == b'ANC:1\t20\t20\t10\t0.5\nCNA:3\t20\t20\t10\t0.5\n'


def test_redundancy_across_shapes_and_positions(tmp_path):
    """The parent stands in another shape and at another j; a chain of three; --all keeps them."""
    unit = 'CCGATCTGCC'
    contigs = [('c', unit * 30)]
    bed = [('c', 10 * i + 3, '+') for i in range(30)]            # the A of every GATC, '+' only
    shapes = ['XXX', 'XXXX', 'XXXXX', 'X.XX']
    every = specs(run(tmp_path, contigs, bed, shapes=shapes, min_sites=20, min_fraction=0.4, keep_all=True))
    kept = specs(run(tmp_path, contigs, bed, shapes=shapes, min_sites=20, min_fraction=0.4))
    assert run(tmp_path, contigs, bed, shapes=shapes, min_sites=20, min_fraction=0.4) == MS.brute(contigs, bed, None, 'A', shapes, 20, 0.4)
    # the chain ATC:1 < GATC:2 < GATCT:2: GATC:2's parent stands in another shape at another j, GATCT:2 has both above it
    assert {'ATC:1', 'GAT:2', 'CGA:3', 'GATC:2', 'CGAT:3', 'ATCT:1', 'GATCT:2', 'CGATC:3', 'ANCT:1', 'CNAT:3', 'CNGA:4'} <= set(every)
    assert set(kept) == {'ATC:1', 'GAT:2', 'CGA:3', 'ANCT:1', 'CNAT:3', 'CNGA:4'}
    # gapped parents: ANCT:1 holds ATCT:1, CNAT:3 holds CGAT:3, CNGA:4 holds CCGA:4; none holds GATC:2
    kept = specs(run(tmp_path, contigs, bed, shapes=['X.XX', 'XXXX'], min_sites=20, min_fraction=0.4))
    assert set(kept) == {'ANCT:1', 'CNAT:3', 'CNGA:4', 'GATC:2'}


def test_the_order_with_ties(tmp_path):
    """Ties on nMethylated and on the fraction fall to the shape index, then j, then the letters."""
    contigs = [('c', ('CCAGC' * 20) + ('GGACG' * 20))]
    bed = [('c', 5 * i + 2, '+') for i in range(10)] + [('c', 100 + 5 * i + 2, '+') for i in range(10)]
    got = specs(run(tmp_path, contigs, bed, shapes=['XX', 'X.X'], min_sites=10, min_fraction=0.25, keep_all=True))
    assert got == specs(MS.brute(contigs, bed, None, 'A', ['XX', 'X.X'], 10, 0.25, True))
    # all 10 of 20: shape 0 before shape 1, j = 0 before j = 1, the letters in order
    assert got == ['AC:1', 'AG:1', 'CA:2', 'GA:2', 'ANC:1', 'ANG:1', 'CNA:3', 'GNA:3']


@pytest.mark.parametrize('line,what', [
    ('c\t1\t2\tx\t0.5\n', 'fields'), ('c\tone\t2\tx\t0.5\t+\t3\n', 'invalid literal'), ('c\t1\t2\tx\t0.5\t.\t3\n', 'strand'),
    ('d\t1\t2\tx\t0.5\t+\t3\n', 'not in the reference'), ('c\t4\t5\tx\t0.5\t+\t3\n', 'outside'), ('c\t-1\t0\tx\t0.5\t+\t3\n', 'outside'),
    ('\n', 'fields')])
def test_every_value_error(tmp_path, line, what):
    ref = str(tmp_path / 'r.fa')
    open(ref, 'w').write('>c\nACGT\n')
    good, bad = str(tmp_path / 'good.bed'), str(tmp_path / 'bad.bed')
    open(good, 'w').write('c\t0\t1\tx\t0.5\t+\t3\n')
    open(bad, 'w').write('c\t0\t1\tx\t0.5\t+\t3\n' + line)
    with pytest.raises(ValueError, match=what):
        FM.find_motifs(ref, bad, out=str(tmp_path / 'o'))
    with pytest.raises(ValueError, match=what):
        FM.find_motifs(ref, good, bad, out=str(tmp_path / 'o'))
    assert FM.find_motifs(ref, good, good, out=str(tmp_path / 'o')) == 0


@pytest.mark.parametrize('shapes', ['X', '.XX', 'XX.', 'XxX', 'X' * 9, 'X' + '.' * 23 + 'X', 'XX,XX', ''])
def test_bad_shapes(tmp_path, shapes):
    with pytest.raises(ValueError, match='shape'):
        FM.parse_shapes(shapes)


def test_last_record_of_an_id_counts_and_no_rows_is_an_empty_file(tmp_path):
    ref, bed, out = str(tmp_path / 'r.fa'), str(tmp_path / 'b.bed'), str(tmp_path / 'o.tsv')
    open(ref, 'w').write('>c first\nTTTTTTTT\n>c second\nGATCGATC\n')
    open(bed, 'w').write('c\t1\t2\tx\t0.5\t+\t3\nc\t5\t6\tx\t0.5\t+\t3\n')
    assert FM.find_motifs(ref, bed, shapes='XXXX', min_sites=2, out=out) == 1
    assert open(out, 'rb').read() == b'GATC:2\t4\t4\t2\t0.5\n'
    open(out, 'w').write('stale')
    assert FM.find_motifs(ref, bed, shapes='XXXX', out=out) == 0 and open(out, 'rb').read() == b''


@pytest.fixture(scope='module')
def planted():
    return MS.planted_case()


def test_planted_gatc_is_the_first_row(tmp_path, planted):
    """6 * 10^4 random bases, GATC fully methylated at 90 % coverage, 2 % false calls: the first row is GATC:2 and no row holds it."""
    contigs, bed, control = planted
    rows = run(tmp_path, contigs, bed, control).decode().splitlines()
    assert rows[0].split('\t')[0] == 'GATC:2'
    nG, nC, nM = (int(v) for v in rows[0].split('\t')[1:4])
    assert nM == nC and 0.85 * nG < nC < 0.95 * nG and nG > 300
    for row in rows[1:]:
        motif, idx = row.split('\t')[0].split(':')
        at = motif.find('GATC')
        assert not (at >= 0 and at + 2 == int(idx)), row


def test_cli_spec_round_trip_and_root_wrapper(tmp_path, capfd, planted):
    contigs, bed, control = planted
    ref, pb, pc = files(tmp_path, contigs, bed, control, form='vo')
    FM.main(['-r', ref, '--bed', pb, '--control', pc, '--shapes', 'XXXX,XXX.....XXX', '--min_sites', '10', '--min_fraction', '0.2', '--all'])
    text = capfd.readouterr().out
    want = run(tmp_path, contigs, bed, control, shapes=['XXXX', 'XXX.....XXX'], min_sites=10, min_fraction=0.2, keep_all=True).decode()
    assert text == want and text
    for row in text.splitlines()[:8]:
        spec = row.split('\t')[0]
        parsed = refmark.parse_motifs(spec, 'A')
        assert parsed.text == spec
    out = str(tmp_path / 'w.tsv')
    subprocess.check_call([sys.executable, os.path.join(H.REPO, 'find_motifs.py'), '-r', ref, '--bed', pb, '--control', pc, '-b', 'a', '-o', out])
    assert open(out).read().split('\t')[0] == 'GATC:2'
