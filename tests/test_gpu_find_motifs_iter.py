"""find_motifs --iterative on the GPU (mcaller_amd/csrc/motifs/mc_motifiter.inc; Device.motif_report(iterative=True),
find_motifs.find_motifs_device(iterative=True)) against the host statement: the same rows and the same --unexplained file, text
to text and file to file, made by the device, and the same rounds, explained and left-over candidates."""
import os
import random
import subprocess
import sys

import pytest

from mcaller_amd import _lib
from mcaller_amd import find_motifs as FM
from tests import helpers as H
from tests import motif_iter_cases as TC
from tests import motif_iupac_cases as IC
from tests import motif_sites as MS

pytestmark = pytest.mark.gpu

CASES = TC.cases()
WIDE = 'XX' + '.' * 20 + 'XX'                    # 24 wide: the widest shape there is


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def write(tmp_path, contigs, bed, control):
    ref, pb, pc = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), None
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(MS.bed_text(bed))
    if control is not None:
        pc = str(tmp_path / 'control.bed')
        open(pc, 'wb').write(MS.bed_text(control))
    return ref, pb, pc


def device_makes_it(dev, tmp_path, contigs, bed, control=None, what='', **kw):
    """The device's rows and left-over sites, text to text (Device.motif_report) and file to file (find_motifs_device), equal the
    host statement's, and so do its figures -> (the host's rows, its --unexplained file, last_counts, the three stats)."""
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    paths = [str(tmp_path / name) for name in ('host.tsv', 'host.bed', 'out.tsv', 'out.bed')]
    n = FM.find_motifs(ref, pb, pc, out=paths[0], unexplained=paths[1], iterative=True, **kw)
    want, want_left, counts = open(paths[0], 'rb').read(), open(paths[1], 'rb').read(), dict(FM.last_counts)
    dkw = dict(kw)
    dkw['shapes'] = FM.parse_shapes(dkw.pop('shapes', None) or FM.DEFAULT_SHAPES)
    blob, n_rows, reason, left = dev.motif_report(FM.read_reference(ref), text=MS.bed_text(bed),
                                                  control_text=None if control is None else MS.bed_text(control), iterative=True, left=True, **dkw)
    assert reason is None, (what, reason, dev.motif_report_last_stats())
    assert n_rows == n and blob == want and left == want_left, what
    assert FM.find_motifs_device(ref, pb, pc, out=paths[2], unexplained=paths[3], iterative=True, **kw) == n
    assert FM.last_report == dict(by='device', reason=None, n_rows=n), what
    assert open(paths[2], 'rb').read() == want and open(paths[3], 'rb').read() == want_left, what
    st, ist, it = dev.motif_report_last_stats(), dev.motif_report_iupac_last_stats(), dev.motif_report_iter_last_stats()
    print(what, st, ist, it)
    assert st['decline_reason'] == 0 and it['decline_reason'] == 0 and it['decline_line'] == -1 and it['decline_file'] == 0
    assert st['n_rows'] == n and st['n_out_bytes'] == len(want)
    for name in ('n_candidates', 'n_sites', 'n_control', 'n_off_base', 'n_selected'):
        assert st[name] == counts[name], (what, name)
    for name in ('n_rounds', 'n_explained', 'n_unexplained'):
        assert it[name] == counts[name], (what, name)
    if kw.get('iupac'):
        for name in ('n_good', 'n_pure', 'n_maximal'):
            assert ist[name] == counts[name], (what, name)
    assert it['list_bytes'] == 8 * sum(len(seq) for _, seq in dict(contigs).items()) and it['need_bytes'] > it['list_bytes']
    return want, want_left, counts, (st, ist, it)


def specs(text):
    return [line.split('\t')[0] for line in text.decode().splitlines()]


def sites_of(left):
    return [(f[0], int(f[1]), f[5]) for f in (line.split('\t') for line in left.decode().splitlines())]


@pytest.mark.parametrize('iupac', [False, True], ids=['plain', 'iupac'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_the_cases_of_the_host_tests(dev, tmp_path, name, iupac):
    """Among them a palindromic motif (gatcn, three_motifs: both strands of one GATC are explained in one round) and second-round
    motifs that share candidates with the first: GAY then CAC (shared_member, --iupac), GATC then GATTC (three_motifs, plain)."""
    contigs, bed, control, kw = CASES[name]
    want, _, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, control, name, iupac=iupac, **kw)
    assert counts['n_rounds'] == len(want.splitlines()) and (want or (name, iupac) == ('sum_reaches', False))      # (no member reaches alone)
    if name == 'shared_member' and iupac:
        assert specs(want)[:2] == ['GAY:2', 'CAC:2']
    if name == 'three_motifs' and not iupac:
        assert specs(want)[0] == 'GATC:2' and 'GATTC:2' in specs(want)[1:]


def edge_genome(seed, spoil=()):
    """One contig (its base p is bit p % 64 of a plane word: contigs begin at multiples of 64).  A unit of 24 bases, CA, twenty
    letters that differ from unit to unit, GT, is planted so that its first X, its called A and its last X each stand on bit 0, on
    bit 63 and across a word edge -- and the same for the reverse complement's, read on '-'.  The A of every unit is methylated.
    spoil: {unit number: (offset in the unit, letter)}."""
    rng = random.Random(seed)
    starts = [0, 63, 62, 41, 40] + [0, 63, 41, 40, 42]                  # p % 64 of a unit's first base; the last five are read on '-'
    s = list(MS.random_genome(seed, [128 * (len(starts) + 1)], letters='CGT')[0][1])       # no A, and so no T either, but the units'
    s = [ch if ch != 'T' else 'G' for ch in s]
    bed = []
    for u, r in enumerate(starts):
        unit = 'CA' + ''.join(rng.choice('ACGT') for _ in range(20)) + 'GT'
        if u in spoil:
            unit = unit[:spoil[u][0]] + spoil[u][1] + unit[spoil[u][0] + 1:]
        at = 128 * u + 64 + r
        if u < 5:
            s[at:at + 24] = unit
            bed.append(('edge', at + 1, '+'))
        else:
            s[at:at + 24] = MS.revcomp(unit)
            bed.append(('edge', at + 22, '-'))
    contigs = [('edge', ''.join(s))]
    control = [site for site in MS.candidates(contigs, 'A') if site not in set(bed)]
    return contigs, bed, control


@pytest.mark.parametrize('iupac', [False, True], ids=['plain', 'iupac'])
def test_occurrences_on_the_edges_of_the_plane_words(dev, tmp_path, iupac):
    contigs, bed, control = edge_genome(41)
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, control, 'edges', shapes=[WIDE], min_sites=5, iupac=iupac)
    first = want.decode().splitlines()[0].split('\t')
    assert (iupac or first[0] == 'CA' + 'N' * 20 + 'GT:2') and int(first[3]) >= 10 and left == b''


def test_a_reference_n_under_a_dot_and_under_an_x(dev, tmp_path):
    """Unit 1 has an N among its free letters: explained.  Units 2 and 7 have it under the last and the first X: their windows do
    not count, their sites are left."""
    contigs, bed, control = edge_genome(42, {1: (9, 'N'), 2: (23, 'N'), 7: (0, 'N')})
    assert contigs[0][1].count('N') == 3
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, control, 'N', shapes=[WIDE], min_sites=5)
    assert int(want.decode().splitlines()[0].split('\t')[3]) == 8 and sites_of(left) == sorted([bed[2], bed[7]], key=lambda s: s[1])


def test_a_window_that_leaves_its_contig_by_one_base_is_not_explained(dev, tmp_path):
    """Forty short contigs: GATC at the very start and the very end of the even ones, ATC and GAT -- a GATC less one base -- there
    in the odd ones.  Every A in front of a T is methylated; the truncated ones are what is left."""
    rng = random.Random(43)
    contigs, bed, cut = [], [], []
    for i in range(40):
        mid = ''.join(rng.choice('CG') for _ in range(5 + i))
        seq = ('GATC' + mid + 'GATC') if i % 2 == 0 else ('ATC' + mid + 'GAT')
        name = 'c%d' % i
        contigs.append((name, seq))
        if i % 2 == 0:
            bed += [(name, 1, '+'), (name, 2, '-'), (name, len(seq) - 3, '+'), (name, len(seq) - 2, '-')]
        else:
            cut += [(name, 0, '+'), (name, 1, '-'), (name, len(seq) - 2, '+'), (name, len(seq) - 1, '-')]
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed + cut, None, 'forty contigs', shapes=['XXXX'], min_sites=30)
    assert specs(want) == ['GATC:2'] and counts['n_explained'][0] == len(bed)
    # GAT at an end is half of a GATC on '-' too: (name, len - 1, '-') reads ATC.; none of the four has its window
    assert set(sites_of(left)) == set(cut) and counts['n_unexplained'] == len(cut)


def test_a_motif_that_overlaps_itself(dev, tmp_path):
    """AA in runs of A: every A but a run's last is an occurrence's called letter, and each is explained once."""
    rng = random.Random(44)
    seq = ''.join(rng.choice(['AAAAAAA', 'AAA', 'C', 'G', 'CG', 'AC']) for _ in range(300))
    contigs = [('runs', seq)]
    bed = [s for s in MS.candidates(contigs, 'A') if s[2] == '+' and seq[s[1] + 1:s[1] + 2] == 'A']
    control = [s for s in MS.candidates(contigs, 'A') if s not in set(bed)]
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, control, 'AA', shapes=['XX', 'XXX'], min_sites=5)
    assert specs(want)[0] == 'AA:1' and counts['n_explained'][0] == len(bed) and left == b''


@pytest.mark.parametrize('iupac', [False, True], ids=['plain', 'iupac'])
def test_counters_of_both_placements_are_taken_back(dev, tmp_path, monkeypatch, iupac):
    monkeypatch.setenv('MCALLER_MOTIF_STRETCH', '64')
    contigs, bed, control, kw = CASES['three_motifs']
    _, _, counts, (st, _, _) = device_makes_it(dev, tmp_path, contigs, bed, control, 'stretch 64', iupac=iupac, **kw)
    # 256 entries of XXXXX > 128 slots, 64 of XXXX and of XX..XX
    assert st['stretch'] == 64 and st['n_tables_global'] == 5 and st['n_tables_lds'] == 8 and counts['n_rounds'] >= 3


def test_a_counter_beyond_sixteen_bits_is_taken_back(dev, tmp_path):
    """AA stands 69999 times in 70000 A: round 1 removes them all, and round 2 finds the one candidate that is left, the last A,
    as the second letter of AA."""
    n = 70000
    contigs = [('poly', 'A' * n)]
    bed = [('poly', p, '+') for p in range(n) if p % 3 != 1] + [('poly', n - 1, '+')]
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, None, 'poly', shapes=['XX'], min_sites=1)
    assert specs(want) == ['AA:1', 'AA:2'] and counts['n_explained'] == [n - 1, 1] and left == b''


def test_a_genome_of_a_million_bases(dev, tmp_path):
    """Thousands of workgroups of km_explain on every part of the chip: an explain test that restated ms_key's letters lost a
    varying half per cent of the candidates at this size and none at 10^5 bases."""
    rng = random.Random(45)
    seq = ''.join(rng.choices('ACGT', k=1200000))
    contigs = [('big', seq)]
    bed = IC.sites_matching(contigs, 'GATC', 1)
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, None, 'big', shapes=['XXXX'])
    assert specs(want) == ['GATC:2'] and counts['n_explained'] == [len(bed)] and len(bed) > 9000 and left == b''


def test_one_row_and_sixty_four(dev, tmp_path):
    contigs, bed, control, kw = CASES['gantc']
    four, _, _, _ = device_makes_it(dev, tmp_path, contigs, bed, control, '64', max_motifs=64, **kw)
    one, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, control, '1', max_motifs=1, **kw)
    assert len(four.splitlines()) == 4 and one == four.splitlines(True)[0] and counts['n_unexplained'] == len(left.splitlines()) > 0


def test_a_run_that_ends_in_round_one(dev, tmp_path):
    contigs = MS.random_genome(4, [300])
    bed = MS.candidates(contigs, 'A')[:3]
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, bed, None, 'no row', shapes=['XXX'])
    assert want == b'' and len(left.splitlines()) == 3 and counts['n_rounds'] == 0
    want, left, counts, _ = device_makes_it(dev, tmp_path, contigs, [], None, 'no site', shapes=['XXX'], iupac=True)
    assert want == b'' and left == b''


def test_a_call_without_iterative_behind_one_with(dev, tmp_path):
    """Two calls on one context: the second finds nothing of the first -- its rows are the plain call's, and the left-over planes
    and the rounds are gone."""
    contigs, bed, control, kw = CASES['three_motifs']
    device_makes_it(dev, tmp_path, contigs, bed, control, 'first', iupac=True, **kw)
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    for iupac in (True, False):
        n = FM.find_motifs(ref, pb, pc, out=str(tmp_path / 'host.tsv'), iupac=iupac, **kw)
        blob, n_rows, reason = dev.motif_report(FM.read_reference(ref), text=MS.bed_text(bed), control_text=MS.bed_text(control), iupac=iupac, **kw)
        assert reason is None and n_rows == n >= 3 and blob == open(str(tmp_path / 'host.tsv'), 'rb').read()
        it = dev.motif_report_iter_last_stats()
        assert it['n_rounds'] == 0 and it['n_explained'] == [] and it['list_bytes'] == 0
        with pytest.raises(RuntimeError):
            dev._motif_left([name for name, _ in contigs], None)


def test_too_little_memory_for_the_list_declines(dev, tmp_path, monkeypatch):
    """One byte less than the call counts: the plain call, which needs no list, still fits."""
    contigs, bed, control, kw = CASES['gantc']
    _, _, _, (_, _, it) = device_makes_it(dev, tmp_path, contigs, bed, control, 'memory enough', **kw)
    monkeypatch.setenv('MCALLER_MOTIF_DEVICE_BYTES', str(it['need_bytes'] - 1))
    blob, n_rows, reason, left = dev.motif_report(dict(contigs), text=MS.bed_text(bed), iterative=True, left=True, **kw)
    st, it2 = dev.motif_report_last_stats(), dev.motif_report_iter_last_stats()
    assert blob is None and left is None and n_rows == 0 and 'do not fit' in reason
    assert st['decline_reason'] == it2['decline_reason'] == _lib.MOTIF_DECLINE['memory'] and it2['need_bytes'] == it['need_bytes']
    blob, _, reason = dev.motif_report(dict(contigs), text=MS.bed_text(bed), **kw)
    assert reason is None and blob is not None                        # the plain call fits: it was the list and the left-over planes
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    paths = [str(tmp_path / name) for name in ('host.tsv', 'host.bed', 'out.tsv', 'out.bed')]
    n = FM.find_motifs(ref, pb, pc, out=paths[0], unexplained=paths[1], iterative=True, **kw)
    assert FM.find_motifs_device(ref, pb, pc, out=paths[2], unexplained=paths[3], iterative=True, **kw) == n == 4
    assert FM.last_report['by'] == 'host' and 'do not fit' in FM.last_report['reason']
    assert open(paths[2], 'rb').read() == open(paths[0], 'rb').read() and open(paths[3], 'rb').read() == open(paths[1], 'rb').read()


def child(args, tmp_path, **env):
    done = subprocess.run([sys.executable] + args, env=dict(os.environ, PYTHONPATH=H.REPO, **env), cwd=str(tmp_path), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0, done.stdout.decode('utf-8', 'replace')[-2000:]
    return done.stdout


def test_the_command_line_file_to_file(tmp_path):
    contigs, bed, control, _ = CASES['three_motifs']
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    args = ['-m', 'mcaller_amd.find_motifs', '-r', ref, '--bed', pb, '--control', pc, '--shapes', 'XXXX,XXXXX,XX..XX', '--min_sites', '5', '--iupac',
            '--iterative', '--max_motifs', '8']
    child(args + ['--device', '-o', 'device.tsv', '--unexplained', 'device.bed'], tmp_path)
    child(args + ['-o', 'host.tsv', '--unexplained', 'host.bed'], tmp_path)
    got = open(str(tmp_path / 'device.tsv'), 'rb').read()
    assert got == open(str(tmp_path / 'host.tsv'), 'rb').read() and specs(got)[:2] == ['GATC:2', 'GANTC:2']
    left = open(str(tmp_path / 'device.bed'), 'rb').read()
    assert left == open(str(tmp_path / 'host.bed'), 'rb').read() and left


def test_poisoned_allocations(tmp_path):
    """A process of its own: the library reads MCALLER_POISON once.  Every fresh device block is filled with 0xAB, so a list slot, a
    plane word or a counter that is read before it was written changes the rows or the left-over sites."""
    contigs, bed, control, _ = CASES['three_motifs']
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    out = child([os.path.join(H.REPO, 'tests', '_motif_iter_worker.py'), ref, pb, pc, 'XXXX,XXXXX,XX..XX'], tmp_path, MCALLER_POISON='1')
    assert b'iterative ok' in out, out.decode('utf-8', 'replace')[-2000:]
