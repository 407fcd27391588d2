"""find_motifs --iupac on the GPU (mcaller_amd/csrc/motifs/mc_motifiupac.inc; Device.motif_report(iupac=True),
find_motifs.find_motifs_device(iupac=True)) against the host statement: the same bytes text to text and file to file, made by the
device, and the same counts of good entries, pure and maximal patterns."""
import os
import random
import subprocess
import sys

import pytest

from mcaller_amd import _lib
from mcaller_amd import find_motifs as FM
from tests import helpers as H
from tests import motif_iupac_cases as IC
from tests import motif_sites as MS

pytestmark = pytest.mark.gpu

CASES = IC.cases()


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
    """The device's bytes, text to text (Device.motif_report) and file to file (find_motifs_device), equal the host statement's,
    and so do its counts -> (the host's text, the two stats of the file call)."""
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    host_out, out = str(tmp_path / 'host.tsv'), str(tmp_path / 'out.tsv')
    n = FM.find_motifs(ref, pb, pc, out=host_out, iupac=True, **kw)
    want, counts = open(host_out, 'rb').read(), dict(FM.last_counts)
    dkw = dict(kw)
    dkw['shapes'] = FM.parse_shapes(dkw.pop('shapes', None) or FM.DEFAULT_SHAPES)
    blob, n_rows, reason = dev.motif_report(FM.read_reference(ref), text=MS.bed_text(bed), control_text=None if control is None else MS.bed_text(control),
                                            iupac=True, **dkw)
    assert reason is None, (what, reason, dev.motif_report_last_stats())
    assert n_rows == n and blob == want, what
    assert FM.find_motifs_device(ref, pb, pc, out=out, iupac=True, **kw) == n
    assert FM.last_report == dict(by='device', reason=None, n_rows=n), what
    assert open(out, 'rb').read() == want, what
    st, ist = dev.motif_report_last_stats(), dev.motif_report_iupac_last_stats()
    print(what, st, ist)
    assert st['decline_reason'] == 0 and ist['decline_reason'] == 0 and ist['decline_line'] == -1 and ist['decline_file'] == 0
    assert st['n_rows'] == n and st['n_out_bytes'] == len(want)
    for name in ('n_candidates', 'n_sites', 'n_control', 'n_off_base', 'n_selected'):
        assert st[name] == counts[name], (what, name)
    for name in ('n_good', 'n_pure', 'n_maximal'):
        assert ist[name] == counts[name], (what, name)
    assert ist['lattice_bytes'] >= sum(15 ** (s.count('X') - 1) * s.count('X') for s in dkw['shapes'])
    return want, st, ist


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_cases_of_the_host_tests(dev, tmp_path, name):
    """Among them: a parent lookup where the called base is not the same X in child and parent (gatcn: NGATC:3 of XXXXX is dropped
    for GATC:2 of XXXX), 50625 patterns a table with a ragged last workgroup (XXXXX), 225 (XXX: less than a workgroup)."""
    contigs, bed, control, kw = CASES[name]
    want, _, _ = device_makes_it(dev, tmp_path, contigs, bed, control, name, **kw)
    assert want


def test_a_lattice_of_fifteen_patterns(dev, tmp_path):
    """k = 2: less than a wave; one pass of the transform straight from the good flags into the lattice."""
    contigs = MS.random_genome(3, [600])
    want, _, ist = device_makes_it(dev, tmp_path, contigs, IC.sites_matching(contigs, 'AS', 0), None, 'k = 2', shapes=['XX'], min_sites=2)
    assert want.startswith(b'AS:1\t') and ist['n_maximal'] == 2          # one of either table


def unit_genome(seed, n_units, spacing=400):
    """The full 15^7 lattice with a small box: CAAYGTCAGRTAC in ONE fixed context of 12 bases to either side, planted every `spacing`
    bases with its four (Y, R); the second A of every unit is methylated on '+'.  Every 8-X window around a methylated A lies inside
    the unit, so no X sees more than two letters among the good entries."""
    rng = random.Random(seed)
    s = list(MS.random_genome(seed, [n_units * spacing])[0][1])
    bed = []
    for u in range(n_units):
        unit = 'GGCTTGACCTGA' + 'CAA' + 'CT'[u & 1] + 'GTCAG' + 'AG'[(u >> 1) & 1] + 'TAC' + 'TGGTCCAGTTCG'
        at = u * spacing + rng.randrange(40, spacing - 80)
        s[at:at + len(unit)] = unit
        bed.append(('ctg0', at + 12 + 2, '+'))
    return [('ctg0', ''.join(s))], bed


def test_one_table_set_of_eight_x(dev, tmp_path):
    """XXXX.....XXXX alone: eight lattices of 15^7 = 170 859 375 patterns on the device; the host statement stays in its box."""
    contigs, bed = unit_genome(13, 80)
    control = [s for s in MS.candidates(contigs, 'A') if s[1] % 3 == 0 and s not in set(bed)]
    want, _, ist = device_makes_it(dev, tmp_path, contigs, bed, control, 'k = 8', shapes=['XXXX.....XXXX'])
    assert b'\nCAAYNNNNNRTAC:3\t' in want and ist['lattice_bytes'] > 8 * 15 ** 7


def test_a_noisy_genome_where_the_transform_has_work(dev, tmp_path):
    contigs, bed, control = IC.noisy()
    _, st, ist = device_makes_it(dev, tmp_path, contigs, bed, control, 'noisy', shapes=['XXX', 'XXXX', 'X.X', 'XX.XX', 'XXXXXX'], min_sites=1)
    assert st['n_rows'] >= 50 and ist['n_good'] >= 500 and ist['n_pure'] > ist['n_good']
    device_makes_it(dev, tmp_path, contigs, bed, control, 'noisy, all', shapes=['XXX', 'XXXX', 'X.X', 'XX.XX'], min_sites=1, keep_all=True)


def test_counts_placed_in_global_memory_feed_the_lattice(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_MOTIF_STRETCH', '64')
    contigs, bed, control, kw = CASES['two_shapes']
    _, st, _ = device_makes_it(dev, tmp_path, contigs, bed, control, 'stretch 64', **kw)
    assert st['stretch'] == 64 and st['n_tables_global'] == 5 and st['n_tables_lds'] == 4      # 256 entries of XXXXX > 128 slots, 64 of XX.XX


def test_too_little_memory_for_the_lattices_declines(dev, tmp_path, monkeypatch):
    """Seven lattices of 15^6 bytes: far more than the plain call needs, so one byte less than they need is the lattices' decline."""
    contigs, bed, control, kw = CASES['gantc']
    kw = dict(kw, shapes=['XXX.XXXX'])
    _, _, ist = device_makes_it(dev, tmp_path, contigs, bed, control, 'memory enough', **kw)
    assert ist['lattice_bytes'] > 7 * 15 ** 6
    monkeypatch.setenv('MCALLER_MOTIF_DEVICE_BYTES', str(ist['lattice_bytes'] - 1))
    blob, n_rows, reason = dev.motif_report(dict(contigs), text=MS.bed_text(bed), iupac=True, **kw)
    st, ist2 = dev.motif_report_last_stats(), dev.motif_report_iupac_last_stats()
    assert blob is None and n_rows == 0 and 'do not fit' in reason
    assert st['decline_reason'] == ist2['decline_reason'] == _lib.MOTIF_DECLINE['memory'] and ist2['lattice_bytes'] == ist['lattice_bytes']
    blob, _, reason = dev.motif_report(dict(contigs), text=MS.bed_text(bed), **kw)
    assert reason is None and blob is not None                        # the plain call fits: it was the lattices
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    host_out, out = str(tmp_path / 'host.tsv'), str(tmp_path / 'out.tsv')
    n = FM.find_motifs(ref, pb, pc, out=host_out, iupac=True, **kw)
    assert FM.find_motifs_device(ref, pb, pc, out=out, iupac=True, **kw) == n and n > 0
    assert FM.last_report['by'] == 'host' and 'do not fit' in FM.last_report['reason']
    assert open(out, 'rb').read() == open(host_out, 'rb').read()


def child(args, tmp_path, **env):
    done = subprocess.run([sys.executable] + args, env=dict(os.environ, PYTHONPATH=H.REPO, **env), cwd=str(tmp_path), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0, done.stdout.decode('utf-8', 'replace')[-2000:]
    return done.stdout


def test_the_command_line_file_to_file(tmp_path):
    contigs, bed, control, _ = CASES['member_uncovered']
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    args = ['-m', 'mcaller_amd.find_motifs', '-r', ref, '--bed', pb, '--control', pc, '--shapes', 'XXXX,XXXXX,XX.XX', '--min_sites', '5', '--iupac']
    child(args + ['--device', '-o', 'device.tsv'], tmp_path)
    child(args + ['-o', 'host.tsv'], tmp_path)
    got = open(str(tmp_path / 'device.tsv'), 'rb').read()
    assert got == open(str(tmp_path / 'host.tsv'), 'rb').read() and b'GAHT:2\t' in got and got.startswith(b'GANTC:2\t')


def test_poisoned_allocations(tmp_path):
    """A process of its own: the library reads MCALLER_POISON once.  Every fresh device block is filled with 0xAB, so a flag, a
    scratch byte or a counter that is read before it was written changes the rows."""
    contigs, bed, control = IC.noisy()
    ref, pb, pc = write(tmp_path, contigs, bed, control)
    out = child([os.path.join(H.REPO, 'tests', '_motif_iupac_worker.py'), ref, pb, pc, 'XX,XXX,XX.XX,XXXXXX'], tmp_path, MCALLER_POISON='1')
    assert b'iupac ok' in out, out.decode('utf-8', 'replace')[-2000:]
