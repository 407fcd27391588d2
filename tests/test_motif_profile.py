"""mcaller_amd/motif_profile.py, the host statement (NumPy), against the brute force of tests/profile_cases.py on every case, for the
profile file and the neighbours file; every ValueError of the definition; the command line; --from_report on a file find_motifs
wrote; the sums over contigs against find_motifs' own row."""
import os
import subprocess
import sys

import pytest

from mcaller_amd import find_motifs as FM
from mcaller_amd import motif_profile as MP
from tests import motif_sites as MS
from tests import profile_cases as PC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host(tmp_path, case, **more):
    ref, pb, pc = PC.write(tmp_path, case)
    out, nn = str(tmp_path / 'host.tsv'), str(tmp_path / 'host.nn')
    kw = dict(case.kw, **more)
    n = MP.motif_profile(ref, pb, pc, out=out, nn=nn if kw.get('neighbours') is not None else None, **kw)
    return n, open(out, 'rb').read(), (open(nn, 'rb').read() if kw.get('neighbours') is not None else b'')


@pytest.mark.parametrize('name', [c.name for c in PC.CASES])
def test_host_statement_equals_the_brute_force(tmp_path, name):
    case, want = PC.BY_NAME[name], PC.expected(name)
    n, profile, nn = run_host(tmp_path, case)
    assert profile == want.profile and nn == want.nn and n == want.n_rows
    assert MP.last_counts == dict(n_bins=want.n_bins, n_rows=want.n_rows, n_off_base=want.n_off_base, n_defined=want.n_defined, n_pairs=want.n_pairs)
    assert MP.last_report == dict(by='host', reason='the host statement was asked for', n_rows=want.n_rows, n_nn_rows=len(want.nn_rows))


def test_small_blocks_of_the_distance_loop_change_nothing(tmp_path, monkeypatch):
    case, want = PC.BY_NAME['neighbours_of_65_bins_k_5'], PC.expected('neighbours_of_65_bins_k_5')
    rows = MP.neighbour_rows
    monkeypatch.setattr(MP, 'neighbour_rows', lambda *a, **kw: rows(*a, block=7, **kw))
    assert run_host(tmp_path, case)[2] == want.nn


def test_every_value_error(tmp_path):
    case = PC.BY_NAME['two_motifs_sharing_sites']
    ref, pb, pc = PC.write(tmp_path, case)
    nn = str(tmp_path / 'x.nn')
    ok = dict(motifs='GATC:2', out=str(tmp_path / 'o'))
    assert MP.motif_profile(ref, pb, pc, **ok) == 1
    for bad in (dict(base='N'), dict(motifs=None), dict(from_report=pb), dict(motifs=''), dict(motifs='GATC:1'), dict(motifs='GAXC:2'),
                dict(motifs='GATC:2,gatc'), dict(motifs=','.join(['GATC:2'] + ['A' + 'C' * i for i in range(64)])), dict(motifs='A' * 33),
                dict(motifs=['GATC:2,CA:2']), dict(window=63), dict(window=-1), dict(window=64.0), dict(window=True), dict(min_sites=0),
                dict(min_shared=0), dict(neighbours=3), dict(nn=nn), dict(neighbours=0, nn=nn), dict(neighbours=17, nn=nn),
                dict(neighbours=99, nn=nn), dict(neighbours=2.0, nn=nn)):
        with pytest.raises(ValueError):
            MP.motif_profile(ref, pb, pc, **dict(ok, **bad))
    assert MP.motif_profile(ref, pb, pc, neighbours=16, nn=nn, window=64, **ok) > 1
    assert len(MP.parse_profile_motifs(PC.M64, 'A')) == 64
    for text in ('c\t0\t1\n', 'ctg0\tx\t1\tk\t0.5\t+\n', 'ctg0\t0\t1\tk\t0.5\t.\n', 'nobody\t0\t1\tk\t0.5\t+\n', 'ctg0\t300\t301\tk\t0.5\t+\n'):
        open(pb, 'w').write(text)
        with pytest.raises(ValueError):
            MP.motif_profile(ref, pb, None, **ok)
        open(pc, 'w').write(text)
        open(pb, 'w').write('')
        with pytest.raises(ValueError):
            MP.motif_profile(ref, pb, pc, **ok)


def test_command_line_and_launcher(tmp_path):
    case, want = PC.BY_NAME['min_shared_cuts_some_pairs'], PC.expected('min_shared_cuts_some_pairs')
    ref, pb, pc = PC.write(tmp_path, case)
    out, nn = str(tmp_path / 'o.tsv'), str(tmp_path / 'o.nn')
    argv = ['-r', ref, '--bed', pb, '--control', pc, '--motifs', PC.M5, '--min_sites', '4', '--neighbours', '6', '--nn', nn, '--min_shared', '4']
    assert MP.main(argv + ['-o', out]) == want.n_rows
    assert open(out, 'rb').read() == want.profile and open(nn, 'rb').read() == want.nn
    os.remove(nn)
    got = subprocess.run([sys.executable, os.path.join(REPO, 'motif_profile.py')] + argv, stdout=subprocess.PIPE, check=True)
    assert got.stdout == want.profile and open(nn, 'rb').read() == want.nn
    for bad in (['--neighbours', '3'], ['--nn', nn], ['--motifs', 'A:1', '--from_report', out]):
        with pytest.raises(SystemExit):
            MP.main(['-r', ref, '--bed', pb] + bad)


def test_from_report_and_the_sums_over_contigs_against_find_motifs(tmp_path):
    """Contigs of a planted-GATC genome; find_motifs reports GATC:2 (plain mode).  A window of find_motifs is cut by a contig end
    exactly where the occurrence of the motif is: the shape XXXX is the motif's width, so both rules count the same occurrences,
    and the profile summed over the contigs is find_motifs' row."""
    contigs, bed, control = MS.random_case(77, [4000, 2500, 1500, 300])
    ref, pb, pc = str(tmp_path / 'r.fa'), str(tmp_path / 's.bed'), str(tmp_path / 'c.bed')
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(MS.bed_text(bed))
    open(pc, 'wb').write(MS.bed_text(control))
    report = str(tmp_path / 'motifs.tsv')
    assert FM.find_motifs(ref, pb, pc, shapes=['XXXX'], min_sites=20, out=report) >= 1
    rows = [line.split('\t') for line in open(report).read().splitlines()]
    assert rows[0][0] == 'GATC:2'
    out = str(tmp_path / 'p.tsv')
    MP.motif_profile(ref, pb, pc, from_report=report, out=out)
    got = [line.split('\t') for line in open(out).read().splitlines()]
    assert [r[3] for r in got[:len(rows)]] == [r[0] for r in rows] and MP.last_counts['n_bins'] == 4
    for spec, nG, nC, nM, _ in rows:
        mine = [r for r in got if r[3] == spec]
        assert [sum(int(r[k]) for r in mine) for k in (4, 5, 6)] == [int(nG), int(nC), int(nM)], spec
    want = PC.brute(contigs, bed, control, ','.join(r[0] for r in rows))
    assert open(out, 'rb').read() == want.profile
