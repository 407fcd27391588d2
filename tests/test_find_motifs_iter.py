"""find_motifs --iterative, the host statement, against the brute force of tests/motif_iter_cases.py: the same rows and the same
--unexplained file in both modes; the properties the definition states; and without --iterative the bytes and counts of before."""
import pytest

from mcaller_amd import find_motifs as FM
from tests import motif_iter_cases as TC
from tests import motif_sites as MS

CASES = TC.cases()


def write(tmp_path, contigs, bed, control):
    ref, pb, pc = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), None
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(MS.bed_text(bed))
    if control is not None:
        pc = str(tmp_path / 'control.bed')
        open(pc, 'wb').write(MS.bed_text(control))
    return ref, pb, pc


def run(tmp_path, contigs, bed, control, **kw):
    """-> (the rows, the --unexplained file or None, the row count, last_counts) through the files."""
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    out, left = str(tmp_path / 'out.tsv'), str(tmp_path / 'left.bed')
    if kw.get('iterative'):
        kw = dict(kw, unexplained=left)
    n = FM.find_motifs(ref, pb, pc, out=out, **kw)
    assert FM.last_report == dict(by='host', reason='the host statement was asked for', n_rows=n)
    return open(out, 'rb').read(), (open(left, 'rb').read() if kw.get('iterative') else None), n, dict(FM.last_counts)


_RESULTS = {}


def result(name, iupac, tmp_path):
    """The host statement's and the brute force's answers for a case, computed once."""
    if (name, iupac) not in _RESULTS:
        contigs, bed, control, kw = CASES[name]
        _RESULTS[name, iupac] = (run(tmp_path, contigs, bed, control, iupac=iupac, iterative=True, **kw),
                                 TC.brute_iterative(contigs, bed, control, iupac=iupac, **kw))
    return _RESULTS[name, iupac]


@pytest.mark.parametrize('iupac', [False, True], ids=['plain', 'iupac'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_the_host_statement_is_the_brute_force(tmp_path, name, iupac):
    (text, left, n, counts), (want, want_explained, want_left) = result(name, iupac, tmp_path)
    assert text == want and n == len(want.splitlines()) == counts['n_rounds']
    assert counts['n_explained'] == want_explained and left == want_left
    assert counts['n_unexplained'] == len(want_left.splitlines())


@pytest.mark.parametrize('iupac', [False, True], ids=['plain', 'iupac'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_what_the_definition_promises(tmp_path, name, iupac):
    """A row's nGenome is what it explains; n_unexplained is round 1's methylated candidates less the rows' nMethylated; the figures
    of round 1 are the plain call's; the first line is the plain call's first line."""
    contigs, bed, control, kw = CASES[name]
    (text, left, n, counts), _ = result(name, iupac, tmp_path)
    rows = [line.split('\t') for line in text.decode().splitlines()]
    assert [int(r[1]) for r in rows] == counts['n_explained'] and all(int(r[1]) >= 1 for r in rows)
    once, _, _, once_counts = run(tmp_path, contigs, bed, control, iupac=iupac, **kw)
    for key in once_counts:
        assert counts[key] == once_counts[key], key
    base = kw.get('base', 'A')
    n_meth = len(set(bed) & set(MS.candidates(contigs, base)))
    assert n_meth == counts['n_sites'] - len(set(bed) - set(MS.candidates(contigs, base)))
    assert counts['n_unexplained'] == n_meth - sum(int(r[3]) for r in rows)
    assert text[:text.find(b'\n') + 1] == once[:once.find(b'\n') + 1]
    one, _, n_one, one_counts = run(tmp_path, contigs, bed, control, iupac=iupac, iterative=True, max_motifs=1, **kw)
    assert one == once[:once.find(b'\n') + 1] and n_one == one_counts['n_rounds'] == len(one.splitlines())


def test_the_rounds_the_issue_names(tmp_path):
    specs = lambda text: [line.split('\t')[0] for line in text.decode().splitlines()]
    assert len(specs(result('gantc', False, tmp_path)[0][0])) == 4
    assert specs(result('shared_member', True, tmp_path)[0][0])[:2] == ['GAY:2', 'CAC:2']
    assert specs(result('base_c', False, tmp_path)[0][0])[:2] == ['CCAGG:2', 'CCTGG:2']
    three = specs(result('three_motifs', True, tmp_path)[0][0])
    plain = specs(result('three_motifs', False, tmp_path)[0][0])
    assert three[:2] == ['GATC:2', 'GANTC:2'] and len(three) == 3 and three[2].startswith('CCAA')
    assert len(plain) == 6 and plain[0] == 'GATC:2' and 'GATTC:2' in plain[1:]


def test_a_second_round_motif_that_shares_candidates_with_the_first(tmp_path):
    """GAY then CAC of XXX: the A of GACAC is a candidate of both; GAY takes it, and CAC's counts in round 2 are without it."""
    contigs, bed, control, kw = CASES['shared_member']
    (text, _, _, _), _ = result('shared_member', True, tmp_path)
    once = run(tmp_path, contigs, bed, control, iupac=True, **kw)[0]
    cac_once = [line for line in once.decode().splitlines() if line.startswith('CAC:2\t')]
    cac = [line for line in text.decode().splitlines() if line.startswith('CAC:2\t')]
    assert cac and (not cac_once or int(cac[0].split('\t')[1]) < int(cac_once[0].split('\t')[1]))


def test_the_unexplained_file_is_a_bed_for_another_run(tmp_path):
    """Fed back as --bed with the same control: the figures of round 1 less the explained sites; nothing of it is off base."""
    contigs, bed, control, kw = CASES['three_motifs']
    (text, left, n, counts), _ = result('three_motifs', True, tmp_path)
    assert left and n >= 3
    sites = [(f[0], int(f[1]), f[5]) for f in (line.split('\t') for line in left.decode().splitlines())]
    assert all(int(line.split('\t')[2]) == int(line.split('\t')[1]) + 1 for line in left.decode().splitlines())
    assert sites == sorted(sites, key=lambda s: s[1]) and set(sites) <= set(bed)
    ref, _, pc = write(tmp_path, contigs, bed, control)
    again = str(tmp_path / 'again.tsv')
    open(str(tmp_path / 'left_in.bed'), 'wb').write(left)
    FM.find_motifs(ref, str(tmp_path / 'left_in.bed'), pc, out=again, iupac=True, **kw)
    assert FM.last_counts['n_sites'] == counts['n_unexplained'] == len(sites) and FM.last_counts['n_off_base'] == 0
    assert FM.last_counts['n_candidates'] == counts['n_candidates']
    rows = [line.split('\t') for line in text.decode().splitlines()]
    assert len(sites) == len(set(bed) & set(MS.candidates(contigs, 'A'))) - sum(int(r[3]) for r in rows)


def test_max_motifs_stops_a_run_that_would_go_on(tmp_path):
    contigs, bed, control, kw = CASES['gantc']
    (text, _, n, _), _ = result('gantc', False, tmp_path)
    assert n == 4
    two, left, n_two, counts = run(tmp_path, contigs, bed, control, iterative=True, max_motifs=2, **kw)
    assert n_two == 2 and two == b''.join(text.splitlines(True)[:2]) and counts['n_rounds'] == 2 and len(counts['n_explained']) == 2
    assert counts['n_unexplained'] == len(left.splitlines()) > 0


def test_a_run_that_ends_in_round_one_writes_two_empty_files(tmp_path):
    contigs = MS.random_genome(4, [300])
    text, left, n, counts = run(tmp_path, contigs, [], None, iterative=True, shapes=['XXX'])
    assert (text, left, n) == (b'', b'', 0) and counts['n_rounds'] == 0 and counts['n_explained'] == [] and counts['n_unexplained'] == 0


def test_value_errors_and_the_command_line(tmp_path, capsys):
    contigs, bed, control, kw = CASES['gantc']
    ref, pb, _ = write(tmp_path, contigs, bed, None)
    for bad in (0, 65, -1, 2.5, '3', None, True):
        for fn in (FM.find_motifs, FM.find_motifs_device):
            with pytest.raises(ValueError):
                fn(ref, pb, iterative=True, max_motifs=bad, out=str(tmp_path / 'x'), **kw)
    for fn in (FM.find_motifs, FM.find_motifs_device):
        with pytest.raises(ValueError):
            fn(ref, pb, unexplained=str(tmp_path / 'left'), out=str(tmp_path / 'x'), **kw)
    args = ['-r', ref, '--bed', pb, '--shapes', 'XXXXX', '--min_sites', '5', '-o', str(tmp_path / 'cli.tsv')]
    with pytest.raises(SystemExit):
        FM.main(args + ['--unexplained', str(tmp_path / 'left')])
    assert '--unexplained' in capsys.readouterr().err
    with pytest.raises(ValueError):
        FM.main(args + ['--iterative', '--max_motifs', '0'])
    assert FM.main(args + ['--iterative', '--max_motifs', '64', '--unexplained', str(tmp_path / 'left')]) == 4
    (text, left, _, _), _ = result('gantc', False, tmp_path)
    assert open(str(tmp_path / 'cli.tsv'), 'rb').read() == text and open(str(tmp_path / 'left'), 'rb').read() == left


def test_without_iterative_nothing_changes(tmp_path):
    """The bytes are the brute force's of before and last_counts has the keys of before."""
    for name, iupac, keys in (('gantc', False, 5), ('gatcn', True, 8)):
        contigs, bed, control, kw = CASES[name]
        text, _, n, counts = run(tmp_path, contigs, bed, control, iupac=iupac, **kw)
        if iupac:
            from tests import motif_iupac_cases as IC
            assert text == IC.brute_iupac(contigs, bed, control, **kw)[0]
        else:
            assert text == MS.brute(contigs, bed, control, **kw)
        assert len(counts) == keys and not set(counts) & {'n_rounds', 'n_explained', 'n_unexplained'}
    ref = FM.read_reference(write(tmp_path, *CASES['gantc'][:3])[0])
    meth = FM.read_sites(str(tmp_path / 'sites.bed'), ref)
    assert len(FM.report_rows(ref, ['XXXXX'], 'A', meth, None, 5)) == 3
