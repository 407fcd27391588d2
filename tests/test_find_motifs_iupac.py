"""find_motifs --iupac, the host statement (find_motifs.report_rows(..., iupac=True)), against the brute force of
tests/motif_iupac_cases.py: the same bytes and the same counts of good entries, pure and maximal patterns; the rows the issue names;
every SPEC in the syntax --motifs parses and marking exactly nGenome sites; and without iupac the bytes of before."""
import numpy as np
import pytest

from mcaller_amd import find_motifs as FM
from mcaller_amd import refmark
from tests import motif_iupac_cases as IC
from tests import motif_sites as MS

CASES = IC.cases()


def run(tmp_path, contigs, bed, control, **kw):
    """-> (the host statement's text, its row count, last_counts) through the files, as the command line does it."""
    ref, pb, pc, out = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), None, str(tmp_path / 'out.tsv')
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(MS.bed_text(bed))
    if control is not None:
        pc = str(tmp_path / 'control.bed')
        open(pc, 'wb').write(MS.bed_text(control))
    n = FM.find_motifs(ref, pb, pc, out=out, **kw)
    assert FM.last_report == dict(by='host', reason='the host statement was asked for', n_rows=n)
    return open(out, 'rb').read(), n, dict(FM.last_counts)


def specs(text):
    return [line.split('\t')[0] for line in text.decode().splitlines()]


_RESULTS = {}


def result(name, tmp_path):
    """The host statement's and the brute force's answers for a case, computed once."""
    if name not in _RESULTS:
        contigs, bed, control, kw = CASES[name]
        _RESULTS[name] = (run(tmp_path, contigs, bed, control, iupac=True, **kw), IC.brute_iupac(contigs, bed, control, **kw))
    return _RESULTS[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_host_statement_is_the_brute_force(tmp_path, name):
    (text, n, counts), (want, want_counts) = result(name, tmp_path)
    assert text == want and n == len(want.splitlines())
    assert {k: counts[k] for k in want_counts} == want_counts


def test_gantc_is_one_row_where_the_plain_mode_prints_four(tmp_path):
    contigs, bed, control, kw = CASES['gantc']
    (text, _, _), _ = result('gantc', tmp_path)
    plain = specs(run(tmp_path, contigs, bed, control, **kw)[0])
    assert 'GANTC:2' in specs(text) and 'GANTC:2' not in plain
    assert all('GA%sTC:2' % ch in plain and 'GA%sTC:2' % ch not in specs(text) for ch in 'ACGT')


def test_a_member_below_min_fraction_leaves_the_three_letter_code(tmp_path):
    (text, _, _), _ = result('member_below', tmp_path)
    assert 'GADTC:2' in specs(text) and 'GANTC:2' not in specs(text)


def test_a_member_that_is_never_covered_is_not_good(tmp_path):
    contigs, bed, control, kw = CASES['member_uncovered']
    tables = MS.brute_tables(contigs, bed, control, 'A', kw['shapes'])
    assert tables[0, 1, 'GAGTC'][1:] == [0, 0] and tables[0, 1, 'GAGTC'][0] > 0
    (text, _, _), _ = result('member_uncovered', tmp_path)
    assert 'GAHTC:2' in specs(text) and 'GANTC:2' not in specs(text)


def test_members_that_each_miss_min_sites_reach_it_together(tmp_path):
    contigs, bed, control, kw = CASES['sum_reaches']
    tables = MS.brute_tables(contigs, bed, control, 'A', kw['shapes'])
    members = [tables[0, 1, 'GA%sTC' % ch][2] for ch in 'ACGT']
    assert all(0 < m < 20 for m in members) and sum(members) >= 20
    (text, _, _), _ = result('sum_reaches', tmp_path)
    row = [line for line in text.decode().splitlines() if line.startswith('GANTC:2\t')]
    assert len(row) == 1 and int(row[0].split('\t')[3]) == sum(members)
    assert not [s for s in specs(run(tmp_path, contigs, bed, control, **kw)[0]) if s.startswith('GA') and s.endswith('TC:2')]


def test_gatcn_is_dropped_for_gatc_and_kept_with_all(tmp_path):
    (text, _, _), _ = result('gatcn', tmp_path)
    assert 'GATC:2' in specs(text) and 'GATCN:2' not in specs(text) and 'NGATC:3' not in specs(text)
    (text, _, _), _ = result('gatcn_all', tmp_path)
    assert {'GATC:2', 'GATCN:2', 'NGATC:3'} <= set(specs(text))


def test_gantc_of_the_contiguous_shape_is_dropped_for_the_gapped_one(tmp_path):
    (text, _, _), _ = result('two_shapes', tmp_path)
    rows = text.decode().splitlines()
    assert specs(text).count('GANTC:2') == 1                      # of XX.XX: the N stands under the '.'
    contigs, bed, control, kw = CASES['two_shapes']
    both = specs(run(tmp_path, contigs, bed, control, iupac=True, **dict(kw, keep_all=True))[0])
    assert both.count('GANTC:2') == 2 and len(both) > len(rows)


def test_two_maximal_patterns_that_share_a_member_are_both_printed(tmp_path):
    (text, _, _), _ = result('shared_member', tmp_path)
    assert {'GAY:2', 'SAC:2'} <= set(specs(text))


def test_ties_are_broken_by_the_masks_not_by_the_letters(tmp_path):
    (text, _, _), _ = result('ties', tmp_path)
    rows = [line.split('\t') for line in text.decode().splitlines()]
    assert [r[0] for r in rows[:2]] == ['MAC:2', 'GAG:2'] and rows[0][1:] == rows[1][1:] == ['5', '5', '5', '1.0']


def test_base_c(tmp_path):
    (text, _, _), _ = result('base_c', tmp_path)
    assert 'CCWGG:2' in specs(text)


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_spec_is_a_motif_and_marks_ngenome_sites(tmp_path, name):
    contigs, _, _, kw = CASES[name]
    (text, n, _), _ = result(name, tmp_path)
    assert n > 0
    for line in text.decode().splitlines():
        spec, n_genome = line.split('\t')[0], int(line.split('\t')[1])
        parsed = refmark.parse_motifs(spec, kw.get('base', 'A'))
        assert parsed.text == spec
        marked = 0
        for _, seq in contigs:
            fwd, rev = refmark.methylate_iupac(seq.upper(), parsed)
            marked += fwd.count('M') + rev.count('M')
        assert marked == n_genome, spec


def test_the_noisy_genome_prints_at_least_fifty_rows(tmp_path):
    contigs, bed, control = IC.noisy()
    kw = dict(shapes=['XXX', 'XXXX', 'X.X', 'XX.XX'], min_sites=1)
    text, n, counts = run(tmp_path, contigs, bed, control, iupac=True, **kw)
    want, want_counts = IC.brute_iupac(contigs, bed, control, **kw)
    assert text == want and n >= 50 and counts['n_good'] >= 200
    assert {k: counts[k] for k in want_counts} == want_counts


@pytest.mark.parametrize('name', sorted(CASES))
def test_without_iupac_nothing_changes(tmp_path, name):
    contigs, bed, control, kw = CASES[name]
    text, n, counts = run(tmp_path, contigs, bed, control, **kw)
    ref = {cid: seq.upper() for cid, seq in contigs}

    def as_arrays(sites):
        if sites is None:
            return None
        listed = {cid: (np.zeros(len(seq), dtype=bool), np.zeros(len(seq), dtype=bool)) for cid, seq in contigs}
        for cid, p, strand in sites:
            listed[cid][strand == '-'][p] = True
        return listed
    old = FM.report_rows(ref, kw['shapes'], kw.get('base', 'A'), as_arrays(bed), as_arrays(control), kw.get('min_sites', 20), 0.5, kw.get('keep_all', False))
    assert (text, n) == old[:2] and text == MS.brute(contigs, bed, control, **kw)
    assert sorted(counts) == ['n_candidates', 'n_control', 'n_off_base', 'n_selected', 'n_sites']


def test_the_command_line_takes_iupac(tmp_path):
    contigs, bed, control, kw = CASES['gantc']
    ref, pb, out = str(tmp_path / 'r.fasta'), str(tmp_path / 's.bed'), str(tmp_path / 'o.tsv')
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(MS.bed_text(bed))
    FM.main(['-r', ref, '--bed', pb, '--shapes', 'XXXXX', '--min_sites', '5', '--iupac', '-o', out])
    assert open(out, 'rb').read() == result('gantc', tmp_path)[0][0]
