"""Motifs found on the GPU (mcaller_amd/csrc/motifs/mc_motifscan.hip; Device.motif_report, find_motifs.find_motifs_device) against
the host statement (find_motifs.find_motifs, NumPy): the same bytes text to text and file to file, the figures of the stats, every
decline with its reason, file and line and the host's output or error behind it.
(MC_MOTIF_DECLINE_REFERENCE and _ROWS need 2^31 bases or lines, MC_MOTIF_DECLINE_PRINT a fraction below 1e-29: not run here.)"""
import random

import pytest

from mcaller_amd import _lib
from mcaller_amd import find_motifs as FM
from tests import motif_sites as MS

pytestmark = pytest.mark.gpu

W24_2 = 'X' + '.' * 22 + 'X'
W24_8 = 'X..X..X..X..X..X..X....X'


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def write(tmp_path, contigs, t_bed, t_ctl):
    ref, pb, pc = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), None
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(t_bed)
    if t_ctl is not None:
        pc = str(tmp_path / 'control.bed')
        open(pc, 'wb').write(t_ctl)
    return ref, pb, pc


def host(ref, pb, pc, tmp_path, **kw):
    """-> the host statement's bytes, row count and counts, or the exception it raises."""
    out = str(tmp_path / 'host.tsv')
    try:
        n = FM.find_motifs(ref, pb, pc, out=out, **kw)
    except Exception as e:                        # noqa: BLE001 (whatever the statement raises is the expectation)
        return e
    return open(out, 'rb').read(), n, dict(FM.last_counts)


def device_makes_it(dev, tmp_path, contigs, t_bed, t_ctl=None, what='', **kw):
    """The device's bytes, text to text and file to file, equal the host statement's -> the stats of the file call."""
    ref, pb, pc = write(tmp_path, contigs, t_bed, t_ctl)
    want, n, counts = host(ref, pb, pc, tmp_path, **kw)
    refd = FM.read_reference(ref)
    dkw = dict(kw)
    dkw['shapes'] = FM.parse_shapes(dkw.pop('shapes', None) or FM.DEFAULT_SHAPES)
    blob, n_rows, reason = dev.motif_report(refd, text=t_bed, control_text=t_ctl, **dkw)
    assert reason is None, (what, reason, dev.motif_report_last_stats())
    assert n_rows == n and blob == want, what
    out = str(tmp_path / 'out.tsv')
    assert FM.find_motifs_device(ref, pb, pc, out=out, **kw) == n
    assert FM.last_report == dict(by='device', reason=None, n_rows=n), what
    assert open(out, 'rb').read() == want, what
    st = dev.motif_report_last_stats()
    print(what, st)
    assert st['decline_reason'] == 0 and st['decline_line'] == -1 and st['decline_file'] == 0 and st['n_rows'] == n
    assert st['n_out_bytes'] == len(want) and st['n_bytes1'] == len(t_bed) and st['n_bytes2'] == (0 if t_ctl is None else len(t_ctl))
    for name in ('n_candidates', 'n_sites', 'n_control', 'n_off_base', 'n_selected'):
        assert st[name] == counts[name], (what, name)
    assert st['n_tables_lds'] + st['n_tables_global'] == sum(s.count('X') for s in dkw['shapes'])
    return st


def listed(contigs, seed, p_bed=0.5, p_ctl=0.3, base='A'):
    rng = random.Random(seed)
    bed, ctl = [], []
    for site in MS.candidates(contigs, base):
        r = rng.random()
        if r < p_bed:
            bed.append(site)
        elif r < p_bed + p_ctl:
            ctl.append(site)
    rng.shuffle(bed)
    return bed, ctl


def test_placed_cases(dev, tmp_path):
    contigs, bed, control, shapes = MS.placed_case()
    for kw in (dict(min_sites=1, min_fraction=0.0, keep_all=True), dict(min_sites=2, min_fraction=0.3), dict(min_sites=0, min_fraction=0.0, keep_all=True)):
        st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed, 'vo'), MS.bed_text(control), 'placed', shapes=shapes, **kw)
        assert st['n_off_base'] == 4 and st['n_rows'] > 0
        device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), None, 'placed, no control', shapes=shapes, **kw)


def test_stretch_edges(dev, tmp_path, monkeypatch):
    """The smallest stretch, 64 bases.  On the device contig 0 begins at base index 64 and every later contig at the next multiple
    of 64 that leaves 32 bases of padding, so a first contig of 192 bases ends exactly on a stretch boundary.  The genomes are random
    and every candidate is in one of the files or in neither: windows of 2 to 24 bases start, end and straddle every boundary on
    both strands."""
    monkeypatch.setenv('MCALLER_MOTIF_STRETCH', '64')
    contigs = MS.random_genome(11, [192, 700, 64, 33])
    bed, ctl = listed(contigs, 12)
    bed += [('ctg0', 0, '+' if contigs[0][1][0] == 'A' else '-')] if contigs[0][1][0] in 'AT' else []
    shapes = ['XX', 'XXXX', 'X.....X', W24_2, 'XX' + '.' * 20 + 'XX']
    for ctl_text in (MS.bed_text(ctl), None):
        st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), ctl_text, 'stretch 64', shapes=shapes, min_sites=0, min_fraction=0.0, keep_all=True)
        assert st['stretch'] == 64 and st['n_stretches'] == (64 + 256 + 768 + 128 + 128) // 64
        assert st['n_tables_global'] == 0 and st['n_rows'] > 100
    monkeypatch.setenv('MCALLER_MOTIF_STRETCH', '100')           # rounded up to whole words
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(ctl), 'stretch 128', shapes=shapes, min_sites=3)
    assert st['stretch'] == 128


def test_one_kmer_more_than_65535_times(dev, tmp_path):
    """70 000 A: one counter of XXX and of an 8-X shape beyond 2^16 (and, complemented, nothing on '-')."""
    contigs = [('polyA', 'A' * 70000), ('other', 'ACGTTTTTTTTTTTTTGCA')]
    bed = [('polyA', p, '+') for p in range(0, 70000, 7)]
    ctl = [('polyA', p, '+') for p in range(1, 70000, 7)]
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(ctl), 'poly-A', shapes=['XXX', 'XXXXXXXX'], min_sites=1, min_fraction=0.0, keep_all=True)
    ref, pb, pc = write(tmp_path, contigs, MS.bed_text(bed), MS.bed_text(ctl))
    rows = {r.split('\t')[0]: int(r.split('\t')[1]) for r in host(ref, pb, pc, tmp_path, shapes=['XXX', 'XXXXXXXX'], min_sites=1, min_fraction=0.0, keep_all=True)[0].decode().splitlines()}
    assert rows['AAA:2'] > 65535 and rows['AAAAAAAA:4'] > 65535 and st['n_tables_global'] == 0


def test_both_table_placements(dev, tmp_path, monkeypatch):
    """Shapes of 2, 7 and 8 X in one call at a stretch of 4096 bases: the 8-X tables have 16384 used entries, more than the 8192
    candidate slots of a stretch, and are counted in global memory; the others in LDS."""
    monkeypatch.setenv('MCALLER_MOTIF_STRETCH', '4096')
    contigs, bed, control = MS.random_case(21, [15000, 6000], 'A', 'GATC', 1, True)
    shapes = ['XX', 'XXX...XXXX', 'XXXX....XXXX']
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(control), 'placements', shapes=shapes, min_sites=2, min_fraction=0.3)
    assert (st['n_tables_lds'], st['n_tables_global'], st['stretch']) == (9, 8, 4096) and st['n_rows'] > 0
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(control), 'placements, all', shapes=shapes, min_sites=1, min_fraction=0.0, keep_all=True)
    assert st['n_rows'] > 1000
    monkeypatch.delenv('MCALLER_MOTIF_STRETCH')
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(control), 'all in LDS', shapes=shapes, min_sites=2, min_fraction=0.3)
    assert (st['n_tables_lds'], st['n_tables_global']) == (17, 0) and st['stretch'] == 21184      # the whole genome with its padding


def test_width_24_windows_at_every_word_phase(dev, tmp_path):
    """Windows of 24 bases begin at every phase of the 64-base words (a random genome: a candidate at every phase), on both strands."""
    contigs = MS.random_genome(31, [1500, 900])
    bed, ctl = listed(contigs, 32, 0.6, 0.2)
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(ctl), 'width 24', shapes=[W24_2, W24_8, 'XXX..................XXX'],
                         min_sites=0, min_fraction=0.0, keep_all=True)
    assert st['n_rows'] > 1500
    device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(ctl), 'width 24, C', shapes=[W24_2, W24_8], base='C', min_sites=0, keep_all=True)


def forty_contigs():
    contigs = [('contig_%s_x' % (chr(ord('A') + i) if i < 26 else chr(ord('a') + i - 26)), seq) for i, (_, seq) in enumerate(MS.random_genome(41, [120 + i for i in range(40)]))]
    bed, ctl = listed(contigs, 42)
    return contigs, bed, ctl


def test_contig_ids_that_differ_in_one_byte_in_long_probe_chains(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_MOTIF_HASH_MASK', 'f')
    contigs, bed, ctl = forty_contigs()
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), MS.bed_text(ctl), 'hash mask', shapes=['XX', 'XXXX'], min_sites=3)
    assert st['table_slots'] == 128 and st['n_rows'] > 0


def test_contig_table_forced_too_small_declines(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_MOTIF_TABLE_SLOTS', '8')
    contigs, bed, ctl = forty_contigs()
    t_bed, t_ctl = MS.bed_text(bed), MS.bed_text(ctl)
    blob, n_rows, reason = dev.motif_report(dict(contigs), text=t_bed, control_text=t_ctl, shapes=['XX', 'XXXX'], min_sites=3)
    st = dev.motif_report_last_stats()
    assert blob is None and n_rows == 0 and 'table is full' in reason and '(line' not in reason
    assert (st['decline_reason'], st['decline_file'], st['decline_line'], st['table_slots']) == (_lib.MOTIF_DECLINE['table'], 0, -1, 8)
    ref, pb, pc = write(tmp_path, contigs, t_bed, t_ctl)
    want, n, _ = host(ref, pb, pc, tmp_path, shapes=['XX', 'XXXX'], min_sites=3)
    out = str(tmp_path / 'out.tsv')
    assert FM.find_motifs_device(ref, pb, pc, shapes=['XX', 'XXXX'], min_sites=3, out=out) == n
    assert FM.last_report == dict(by='host', reason=reason, n_rows=n) and open(out, 'rb').read() == want and n > 0


def test_too_little_device_memory_declines(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_MOTIF_DEVICE_BYTES', '1000')
    contigs, bed, ctl = forty_contigs()
    blob, n_rows, reason = dev.motif_report(dict(contigs), text=MS.bed_text(bed), shapes=['XX'])
    st = dev.motif_report_last_stats()
    assert blob is None and 'do not fit' in reason and (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.MOTIF_DECLINE['memory'], 0, -1)
    monkeypatch.setenv('MCALLER_MOTIF_DEVICE_BYTES', str(1 << 30))
    device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), None, 'memory enough', shapes=['XX'], min_sites=3)


def test_many_stage_blocks_and_last_lines_without_newline(dev, tmp_path, monkeypatch):
    contigs, bed, ctl = forty_contigs()
    t_bed, t_ctl = MS.bed_text(bed, 'vo'), MS.bed_text(ctl)
    assert len(t_bed) > 10 * 256 and len(t_ctl) > 10 * 256
    for a, b in ((t_bed[:-1], t_ctl), (t_bed, t_ctl[:-1]), (t_bed[:-1], t_ctl[:-1]), (t_bed[:-1], None), (b'', t_ctl), (t_bed, b''), (b'', b''), (b'', None)):
        device_makes_it(dev, tmp_path, contigs, a, b, 'no newline', shapes=['XXX', 'X.X'], min_sites=2, min_fraction=0.3)
    monkeypatch.setenv('MCALLER_TEXT_STAGE_BYTES', '256')
    device_makes_it(dev, tmp_path, contigs, t_bed, t_ctl, 'stage blocks', shapes=['XXX', 'X.X'], min_sites=2, min_fraction=0.3)


def test_two_calls_on_one_context_leave_nothing_behind(dev, tmp_path):
    contigs, bed, control = MS.random_case(51, [5000, 2500], 'A', 'GATC', 1, True)
    t_bed, t_ctl = MS.bed_text(bed), MS.bed_text(control)
    first = device_makes_it(dev, tmp_path, contigs, t_bed, t_ctl, 'first', min_sites=5, min_fraction=0.5)
    assert first['n_rows'] >= 1
    small = MS.random_genome(52, [400])
    sb, _ = listed(small, 53)
    second = device_makes_it(dev, tmp_path, small, MS.bed_text(sb), None, 'second', shapes=['XX', 'XXXXX'], min_sites=1, min_fraction=0.1, keep_all=True)
    assert second['n_bytes2'] == 0 and second['n_control'] == 0
    again = device_makes_it(dev, tmp_path, contigs, t_bed, t_ctl, 'first again', min_sites=5, min_fraction=0.5)
    assert {k: v for k, v in again.items() if not k.startswith('ms_')} == {k: v for k, v in first.items() if not k.startswith('ms_')}


def test_no_rows(dev, tmp_path):
    contigs = MS.random_genome(61, [500])
    bed, _ = listed(contigs, 62, 0.05, 0.0)
    st = device_makes_it(dev, tmp_path, contigs, MS.bed_text(bed), None, 'no rows', shapes=['XXXX'], min_sites=1000)
    assert st['n_rows'] == 0 and st['n_out_bytes'] == 0 and st['n_selected'] == 0
    st = device_makes_it(dev, tmp_path, [('e', '')], b'', None, 'no bases', shapes=['XXXX'], min_sites=0, min_fraction=0.0)
    assert st['n_rows'] == 0 and st['n_candidates'] == 0


def test_planted_gatc_from_the_device(dev, tmp_path):
    contigs, bed, control = MS.planted_case()
    ref, pb, pc = write(tmp_path, contigs, MS.bed_text(bed), MS.bed_text(control))
    out = str(tmp_path / 'o.tsv')
    FM.main(['-r', ref, '--bed', pb, '--control', pc, '-o', out, '--device'])
    assert FM.last_report['by'] == 'device' and open(out).read().split('\t')[0] == 'GATC:2'
    assert open(out, 'rb').read() == host(ref, pb, pc, tmp_path)[0]


GOOD = 'c\t1\t2\tx\t0.5\t+\t3\n'


def declines():
    """name -> (bed text, control text or None, reason, file, 0-based line in it)."""
    long_line = 'c\t0\t1\t' + 'x' * 66000 + '\t0.5\t+\t3\n'
    return {
        'high_byte_in_an_unused_field': (GOOD + 'c\t0\t1\tx\xe9\t0.5\t+\t3\n', None, 'high_byte', 1, 1),
        'high_byte_in_the_chrom': (GOOD + 'c\xe9\t0\t1\tx\t0.5\t+\t3\n', None, 'high_byte', 1, 1),
        'carriage_returns': (GOOD.replace('\n', '\r\n') * 2, None, 'control', 1, 0),
        'control_byte_in_the_control': (GOOD, GOOD * 3 + 'c\t0\t1\tx\x01\t0.5\t+\t3\n', 'control', 2, 3),
        'long_line': (GOOD + long_line, None, 'long_line', 1, 1),
        'five_fields': (GOOD + 'c\t0\t1\tx\t0.5\n' + 'd\t0\n', GOOD, 'fields', 1, 1),
        'blank_line': (GOOD + '\n' + GOOD, None, 'fields', 1, 1),
        'fields_in_the_control_after_a_bed_without_newline': (GOOD[:-1], GOOD + 'c\t0\t1\n', 'fields', 2, 1),
        'empty_chrom': (GOOD + '\t0\t1\tx\t0.5\t+\t3\n', None, 'field', 1, 1),
        'empty_start': (GOOD + 'c\t\t1\tx\t0.5\t+\t3\n', None, 'field', 1, 1),
        'start_with_a_blank': (GOOD + 'c\t 0\t1\tx\t0.5\t+\t3\n', None, 'field', 1, 1),          # int(' 0') is 0: the host's rows
        'start_with_a_sign': (GOOD + 'c\t-1\t0\tx\t0.5\t+\t3\n', None, 'field', 1, 1),
        'start_not_a_number': (GOOD + 'c\tzero\t1\tx\t0.5\t+\t3\n', None, 'field', 1, 1),
        'bad_strand': (GOOD + 'c\t0\t1\tx\t0.5\t.\t3\n', None, 'field', 1, 1),
        'strand_of_two_bytes': (GOOD + 'c\t0\t1\tx\t0.5\t+-\n', None, 'field', 1, 1),
        'unknown_chrom': (GOOD, 'cc\t0\t1\tx\t0.5\t+\t3\n' + GOOD, 'chrom', 2, 0),
        'start_at_the_contig_length': (GOOD + 'c\t8\t9\tx\t0.5\t+\t3\n', None, 'range', 1, 1),
        'start_of_thirty_digits': (GOOD + 'c\t%s\t9\tx\t0.5\t+\t3\n' % ('9' * 30), None, 'range', 1, 1),
        'the_first_line_and_the_smallest_reason': (GOOD + 'd\t9\t1\tx\t0.5\t+\t3\n' + 'c\t0\n', 'c\t0\n', 'chrom', 1, 1),
    }


DECLINES = declines()


@pytest.mark.parametrize('name', sorted(DECLINES))
def test_every_decline(dev, tmp_path, name):
    t_bed, t_ctl, reason, file, line = DECLINES[name]
    t_bed, t_ctl = t_bed.encode('latin-1'), (None if t_ctl is None else t_ctl.encode('latin-1'))
    contigs = [('c', 'GATCGATC')]
    kw = dict(shapes=['XX', 'XXXX'], min_sites=1, min_fraction=0.0)
    blob, n_rows, why = dev.motif_report(dict(contigs), text=t_bed, control_text=t_ctl, **kw)
    st = dev.motif_report_last_stats()
    print(name, why, st)
    assert blob is None and n_rows == 0 and why
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.MOTIF_DECLINE[reason], file, line)
    assert '(%s)' % ('bed' if file == 1 else 'control') in why and '(line %d)' % (line + 1) in why
    ref, pb, pc = write(tmp_path, contigs, t_bed, t_ctl)
    want = host(ref, pb, pc, tmp_path, **kw)
    out = str(tmp_path / 'out.tsv')
    if isinstance(want, Exception):
        assert isinstance(want, ValueError)
        with pytest.raises(ValueError):
            FM.find_motifs_device(ref, pb, pc, out=out, **kw)
    else:
        assert name in ('high_byte_in_an_unused_field', 'carriage_returns', 'control_byte_in_the_control', 'long_line', 'start_with_a_blank')
        assert FM.find_motifs_device(ref, pb, pc, out=out, **kw) == want[1]
        assert FM.last_report == dict(by='host', reason=why, n_rows=want[1])
        assert open(out, 'rb').read() == want[0] and want[1] > 0
