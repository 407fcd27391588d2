"""The motif profile on the GPU (mcaller_amd/csrc/motifs/mc_motifprofile.inc; Device.motif_profile, motif_profile.motif_profile_device)
against the host statement (motif_profile.motif_profile, NumPy) on every case of tests/profile_cases.py: the same bytes for both
files, text to text and file to file, the figures of the stats against last_counts, every reachable decline with its reason, file
and line and the host's output or error behind it.
(MC_MOTIF_DECLINE_REFERENCE and _ROWS need 2^31 bases or lines, MC_MOTIF_DECLINE_PRINT a fraction or a distance below 1e-29: a
fraction of two 32-bit counts and a mean of differences of such fractions are 0.0 or far above it.  Not run here.)"""
import pytest

from mcaller_amd import _lib
from mcaller_amd import motif_profile as MP
from tests import motif_sites as MS
from tests import profile_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def host(ref, pb, pc, tmp_path, **kw):
    """-> the host statement's two files, its row count, counts and report, or the exception it raises."""
    out, nn = str(tmp_path / 'host.tsv'), str(tmp_path / 'host.nn')
    try:
        n = MP.motif_profile(ref, pb, pc, out=out, nn=nn if kw.get('neighbours') is not None else None, **kw)
    except Exception as e:                        # noqa: BLE001 (whatever the statement raises is the expectation)
        return e
    return open(out, 'rb').read(), (open(nn, 'rb').read() if kw.get('neighbours') is not None else b''), n, dict(MP.last_counts), dict(MP.last_report)


def device_makes_it(dev, tmp_path, case, **more):
    """The device's bytes, text to text and file to file, equal the host statement's -> the stats of the file call."""
    ref, pb, pc = PC.write(tmp_path, case)
    kw = dict(case.kw, **more)
    want, want_nn, n, counts, report = host(ref, pb, pc, tmp_path, **kw)
    dkw = dict(kw)
    base = dkw.pop('base', 'A')
    specs = MP.parse_profile_motifs(dkw.pop('motifs'), base)
    t_bed, t_ctl = MS.bed_text(case.bed), (None if case.control is None else MS.bed_text(case.control))
    blob, n_rows, nn_blob, n_nn_rows, reason = dev.motif_profile(MP.read_reference(ref), text=t_bed, control_text=t_ctl, base=base, specs=specs, **dkw)
    assert reason is None, (case.name, reason, dev.motif_profile_last_stats())
    assert (n_rows, n_nn_rows) == (n, report['n_nn_rows']) and blob == want and nn_blob == want_nn, case.name
    out, nn = str(tmp_path / 'out.tsv'), str(tmp_path / 'out.nn')
    with_nn = kw.get('neighbours') is not None
    assert MP.motif_profile_device(ref, pb, pc, out=out, nn=nn if with_nn else None, **kw) == n
    assert MP.last_report == dict(by='device', reason=None, n_rows=n, n_nn_rows=report['n_nn_rows']), case.name
    assert open(out, 'rb').read() == want and (not with_nn or open(nn, 'rb').read() == want_nn), case.name
    st = dev.motif_profile_last_stats()
    print(case.name, st)
    assert st['decline_reason'] == 0 and st['decline_line'] == -1 and st['decline_file'] == 0
    assert st['n_out_bytes'] == len(want) and st['n_nn_bytes'] == len(want_nn) and st['n_nn_rows'] == report['n_nn_rows']
    assert st['n_bytes1'] == len(t_bed) and st['n_bytes2'] == (0 if t_ctl is None else len(t_ctl))
    for name in ('n_bins', 'n_rows', 'n_off_base', 'n_defined', 'n_pairs'):
        assert st[name] == counts[name], (case.name, name)
    return st


@pytest.mark.parametrize('name', [c.name for c in PC.CASES])
def test_device_equals_the_host_statement(dev, tmp_path, name):
    case = PC.BY_NAME[name]
    st = device_makes_it(dev, tmp_path, case)
    want = PC.expected(name)
    assert st['n_rows'] == want.n_rows and st['n_pairs'] == want.n_pairs          # (and the brute force, by way of the CPU tests)


def test_windows_and_neighbours_of_a_longer_genome(dev, tmp_path):
    """Waves that lie in one bin (the reduced path of the counting kernel) beside waves that do not: contigs of several thousand
    bases under windows of 4096 and of 100 bases, and as whole contigs."""
    contigs, bed, control = MS.random_case(91, [20000, 9000, 4100, 70])
    for window, k in ((4096, 3), (100, 16), (0, 2)):
        case = PC.Case('longer_%d' % window, contigs, bed, control, [], motifs='GATC:2,A:1,CTGCAG:5,RAY:2', window=window, min_sites=3, neighbours=k, min_shared=2)
        st = device_makes_it(dev, tmp_path, case)
        assert st['n_rows'] > 0 and st['n_nn_rows'] > 0


def test_two_calls_on_one_context_leave_nothing_behind(dev, tmp_path):
    a, b = PC.BY_NAME['64_motifs_sparsely_defined'], PC.BY_NAME['overlapping_occurrences']
    first = device_makes_it(dev, tmp_path, a)
    second = device_makes_it(dev, tmp_path, b)
    assert second['n_nn_rows'] == 0 and second['n_pairs'] == 0 and second['nn_lds_bytes'] == 0
    again = device_makes_it(dev, tmp_path, a)
    assert {k: v for k, v in again.items() if not k.startswith('ms_')} == {k: v for k, v in first.items() if not k.startswith('ms_')}
    dev.motif_profile_release()
    device_makes_it(dev, tmp_path, b)


def test_find_motifs_is_as_it_was_beside_a_profile_call(dev, tmp_path):
    from mcaller_amd import find_motifs as FM
    contigs, bed, control = MS.random_case(51, [5000, 2500], 'A', 'GATC', 1, True)
    refd, t_bed, t_ctl = dict(contigs), MS.bed_text(bed), MS.bed_text(control)
    before = dev.motif_report(refd, text=t_bed, control_text=t_ctl, shapes=['XXXX'], min_sites=5)
    st_before = dev.motif_report_last_stats()
    device_makes_it(dev, tmp_path, PC.Case('beside', contigs, bed, control, [], motifs='GATC:2', neighbours=1))
    assert dev.motif_report(refd, text=t_bed, control_text=t_ctl, shapes=['XXXX'], min_sites=5) == before and before[1] >= 1
    st = dev.motif_report_last_stats()
    assert {k: v for k, v in st.items() if not k.startswith('ms_')} == {k: v for k, v in st_before.items() if not k.startswith('ms_')}
    assert FM.MAX_SHAPES == 64


GOOD = 'c\t1\t2\tx\t0.5\t+\t3\n'


def declines():
    """name -> (bed text, control text or None, reason, file, 0-based line in it)."""
    long_line = 'c\t0\t1\t' + 'x' * 66000 + '\t0.5\t+\t3\n'
    return {
        'high_byte': (GOOD + 'c\t0\t1\tx\xe9\t0.5\t+\t3\n', None, 'high_byte', 1, 1),
        'carriage_returns': (GOOD.replace('\n', '\r\n') * 2, None, 'control', 1, 0),
        'control_byte_in_the_control': (GOOD, GOOD * 3 + 'c\t0\t1\tx\x01\t0.5\t+\t3\n', 'control', 2, 3),
        'long_line': (GOOD + long_line, None, 'long_line', 1, 1),
        'five_fields': (GOOD + 'c\t0\t1\tx\t0.5\n' + 'd\t0\n', GOOD, 'fields', 1, 1),
        'fields_in_the_control_after_a_bed_without_newline': (GOOD[:-1], GOOD + 'c\t0\t1\n', 'fields', 2, 1),
        'start_with_a_blank': (GOOD + 'c\t 0\t1\tx\t0.5\t+\t3\n', None, 'field', 1, 1),          # int(' 0') is 0: the host's rows
        'bad_strand': (GOOD + 'c\t0\t1\tx\t0.5\t.\t3\n', None, 'field', 1, 1),
        'unknown_chrom': (GOOD, 'cc\t0\t1\tx\t0.5\t+\t3\n' + GOOD, 'chrom', 2, 0),
        'start_at_the_contig_length': (GOOD + 'c\t8\t9\tx\t0.5\t+\t3\n', None, 'range', 1, 1),
    }


DECLINES = declines()
KW = dict(motifs='GATC:2,A:1', min_sites=1, neighbours=2, min_shared=1)


@pytest.mark.parametrize('name', sorted(DECLINES))
def test_every_decline(dev, tmp_path, name):
    t_bed, t_ctl, reason, file, line = DECLINES[name]
    t_bed, t_ctl = t_bed.encode('latin-1'), (None if t_ctl is None else t_ctl.encode('latin-1'))
    contigs = [('c', 'GATCGATC'), ('d', 'GATCAAAA')]
    specs = MP.parse_profile_motifs(KW['motifs'], 'A')
    blob, n_rows, nn_blob, n_nn_rows, why = dev.motif_profile(dict(contigs), text=t_bed, control_text=t_ctl, specs=specs, min_sites=1, neighbours=2, min_shared=1)
    st = dev.motif_profile_last_stats()
    print(name, why, st)
    assert blob is None and nn_blob is None and n_rows == 0 and n_nn_rows == 0 and why
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.MOTIF_DECLINE[reason], file, line)
    assert '(%s)' % ('bed' if file == 1 else 'control') in why and '(line %d)' % (line + 1) in why
    ref, pb, pc = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), (None if t_ctl is None else str(tmp_path / 'control.bed'))
    open(ref, 'wb').write(MS.fasta(contigs))
    open(pb, 'wb').write(t_bed)
    if pc:
        open(pc, 'wb').write(t_ctl)
    want = host(ref, pb, pc, tmp_path, **KW)
    out, nn = str(tmp_path / 'out.tsv'), str(tmp_path / 'out.nn')
    if isinstance(want, Exception):
        assert isinstance(want, ValueError)
        with pytest.raises(ValueError):
            MP.motif_profile_device(ref, pb, pc, out=out, nn=nn, **KW)
    else:
        assert name in ('high_byte', 'carriage_returns', 'control_byte_in_the_control', 'long_line', 'start_with_a_blank')
        assert MP.motif_profile_device(ref, pb, pc, out=out, nn=nn, **KW) == want[2]
        assert MP.last_report == dict(by='host', reason=why, n_rows=want[2], n_nn_rows=want[4]['n_nn_rows'])
        assert open(out, 'rb').read() == want[0] and open(nn, 'rb').read() == want[1] and want[2] > 0


def test_table_and_memory_declines_and_the_command_line_says_so(dev, tmp_path, monkeypatch, capsys):
    case = PC.BY_NAME['neighbours_of_65_bins_k_5']
    ref, pb, pc = PC.write(tmp_path, case)
    want, want_nn, n, _, _ = host(ref, pb, pc, tmp_path, **case.kw)
    specs = MP.parse_profile_motifs(case.kw['motifs'], 'A')
    dkw = dict(specs=specs, min_sites=2, neighbours=5, min_shared=2)
    monkeypatch.setenv('MCALLER_MOTIF_TABLE_SLOTS', '8')
    got = dev.motif_profile(dict(case.contigs), text=MS.bed_text(case.bed), **dkw)
    st = dev.motif_profile_last_stats()
    assert got[0] is None and 'table is full' in got[4] and '(line' not in got[4]
    assert (st['decline_reason'], st['decline_file'], st['decline_line'], st['table_slots']) == (_lib.MOTIF_DECLINE['table'], 0, -1, 8)
    monkeypatch.delenv('MCALLER_MOTIF_TABLE_SLOTS')
    monkeypatch.setenv('MCALLER_MOTIF_DEVICE_BYTES', '1000')
    got = dev.motif_profile(dict(case.contigs), text=MS.bed_text(case.bed), **dkw)
    st = dev.motif_profile_last_stats()
    assert got[0] is None and 'do not fit' in got[4] and (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.MOTIF_DECLINE['memory'], 0, -1)
    assert st['need_bytes'] > 1000
    out, nn = str(tmp_path / 'o.tsv'), str(tmp_path / 'o.nn')
    argv = ['-r', ref, '--bed', pb, '--motifs', PC.M5, '--min_sites', '2', '--neighbours', '5', '--nn', nn, '-o', out, '--device']
    assert MP.main(argv) == n and MP.last_report['by'] == 'host'
    assert 'do not fit' in capsys.readouterr().err and open(out, 'rb').read() == want and open(nn, 'rb').read() == want_nn
    monkeypatch.setenv('MCALLER_MOTIF_DEVICE_BYTES', str(1 << 30))
    assert MP.main(argv) == n and MP.last_report['by'] == 'device' and capsys.readouterr().err == ''
    assert open(out, 'rb').read() == want and open(nn, 'rb').read() == want_nn
