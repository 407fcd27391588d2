"""The per-site summary of a `.diffs` file made on the GPU (mcaller_amd/csrc/bed/mc_bedsum.hip; make_bed --device) writes the
bytes of make_bed's host code -- itself pinned to the reference's outputs by tests/test_make_bed.py -- and every assertion on
bytes comes with one on WHO made them (make_bed.last_summary): a path that silently falls back proves nothing."""
import contextlib
import io
import json
import os
import shutil
import warnings

import pytest

from tests import bed_files as B
from tests import helpers as H

pytestmark = pytest.mark.gpu

HOST_MADE = {'positions': '-p', 'positions_vo': '-p', 'ref_d2': '--ref', 'gff_vo_d2': '--gff with --vo'}
DEVICE_MADE = ['default_d1', 'default_d3', 'control_d2', 'thresh_d2_t0.7', 'vo_d2', 'gff_d2']


def _main(argv):
    from mcaller_amd import make_bed
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        make_bed.main(argv)
    return buf.getvalue()


@pytest.mark.parametrize('tag', DEVICE_MADE + sorted(HOST_MADE))
def test_reference_goldens(tmp_path, monkeypatch, tag):
    from mcaller_amd import make_bed
    case = json.load(open(os.path.join(H.GOLDEN, 'bed_cases', 'manifest.json')))['cases'][tag]
    shutil.copy(os.path.join(H.GOLDEN, 'bed_cases', 'multi.eventalign.diffs.6'), str(tmp_path / 'multi.eventalign.diffs.6'))
    span = json.load(open(os.path.join(H.GOLDEN, 'testdata', 'rebuilt_fasta_span.json')))
    fasta = str(tmp_path / 'ref.fasta')
    open(fasta, 'w').write('>%s\n%s\n' % (span['contig'], 'N' * span['span_start'] + span['span'] + 'N' * 200))
    args = [{'<POS>': os.path.join(H.GOLDEN, 'bed_cases', 'bed_positions.txt'), '<REF>': fasta}.get(a, a) for a in case['args']]
    monkeypatch.chdir(tmp_path)
    make_bed.last_summary = None
    said = _main(['-f', 'multi.eventalign.diffs.6'] + args + ['--device'])
    assert open(str(tmp_path / case['stem']), 'rb').read() == open(os.path.join(H.GOLDEN, 'bed_cases', case['output']), 'rb').read()
    if case['summary_line']:
        assert case['summary_line'] in said
    if tag in HOST_MADE:
        assert make_bed.last_summary['by'] == 'host' and make_bed.last_summary['reason'] == 'out of scope on the device: ' + HOST_MADE[tag]
    else:
        assert make_bed.last_summary == dict(by='device', reason=None, n_sites=int(case['summary_line'].split()[0]))


@pytest.mark.parametrize('diffs,bed,vo', [
    ('testdata/masonread1.eventalign.diffs.6', 'testdata/masonread1.methylation.summary.bed', False),
    ('testdata/masonread1.eventalign.diffs.6', 'ref_outputs/reference_golden_diffs.vo.bed', True),
    ('ref_outputs/config1_positions_m6A.diffs.6', 'ref_outputs/config1_positions_m6A.bed', False),
    ('ref_outputs/motif_GATC.diffs.6', 'ref_outputs/motif_GATC.bed', False),
    ('ref_outputs/motif_GATC.diffs.6', 'ref_outputs/motif_GATC.vo.bed', True),
])
def test_bed_bytes_on_the_device(tmp_path, monkeypatch, diffs, bed, vo):
    from mcaller_amd import make_bed
    shutil.copy(os.path.join(H.GOLDEN, diffs), str(tmp_path / 'masonread1.eventalign.diffs.6'))
    monkeypatch.chdir(tmp_path)
    make_bed.last_summary = None
    _main(['-f', 'masonread1.eventalign.diffs.6', '-d', '1', '-t', '0.5', '--device'] + (['--vo'] if vo else []))
    assert open(str(tmp_path / 'masonread1.methylation.summary.bed'), 'rb').read() == open(os.path.join(H.GOLDEN, bed), 'rb').read()
    assert make_bed.last_summary['by'] == 'device' and make_bed.last_summary['reason'] is None


def both(tmp_path, text, opts):
    """-> (host bytes, host stdout), (device bytes, device stdout, last_summary) of one text and option set."""
    from mcaller_amd import make_bed
    src = tmp_path / 'case.diffs.6'
    src.write_bytes(text)
    kw = dict(control=opts['control'], with_probs=opts['with_probs'], gff=opts['gff'])
    out = []
    for fn in (make_bed.summarise_diffs, make_bed.summarise_diffs_device):
        dst = tmp_path / ('out.' + fn.__name__)
        buf = io.StringIO()
        make_bed.last_summary = None
        with contextlib.redirect_stdout(buf):
            n = fn(str(src), str(dst), opts['depth'], opts['thresh'], **kw)
        out.append((dst.read_bytes(), buf.getvalue(), n))
    return out[0], out[1], make_bed.last_summary


@pytest.fixture(scope='module')
def host_results(tmp_path_factory):
    """The host function's bytes for every random file, made once (both hash-mask runs compare with them)."""
    from mcaller_amd import make_bed
    d = tmp_path_factory.mktemp('bed_random')
    res = {}
    for seed in range(300):
        text, opts = B.random_case(seed)
        src, dst = d / ('r%d.diffs.6' % seed), d / 'host.out'
        src.write_bytes(text)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            n = make_bed.summarise_diffs(str(src), str(dst), opts['depth'], opts['thresh'], control=opts['control'],
                                         with_probs=opts['with_probs'], gff=opts['gff'])
        res[seed] = (str(src), opts, dst.read_bytes(), buf.getvalue(), n)
    return d, res


@pytest.mark.parametrize('mask', [None, 'f'])
def test_random_files(host_results, monkeypatch, mask):
    """300 generated files of 1-400 rows, options drawn from the in-scope sets: the device's bytes and summary line are the
    host function's, and the device declines none.  MCALLER_BED_HASH_MASK=f leaves 16 hash values: nearly every probe chain
    is long and the byte comparison decides."""
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    if mask:
        monkeypatch.setenv('MCALLER_BED_HASH_MASK', mask)
    else:
        monkeypatch.delenv('MCALLER_BED_HASH_MASK', raising=False)
    d, res = host_results
    longest = 0
    for seed, (src, opts, want, said, n) in res.items():
        dst = d / 'device.out'
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got_n = make_bed.summarise_diffs_device(src, str(dst), opts['depth'], opts['thresh'], control=opts['control'],
                                                    with_probs=opts['with_probs'], gff=opts['gff'])
        assert make_bed.last_summary['by'] == 'device', (seed, make_bed.last_summary)
        assert dst.read_bytes() == want and buf.getvalue() == said and got_n == n, (seed, opts)
        st = get_device().bed_last_stats()
        assert st['n_entries'] == len(B.host_entries(open(src, 'rb').read())) and st['n_sites'] == n
        longest = max(longest, st['longest_probe'])
    if mask:
        assert longest >= 8            # (more than 16 entries on 16 hash values: chains run through other entries' slots)


EDGES = [(name, i) for name, (_, options) in sorted(B.edge_cases().items()) for i in range(len(options))]


@pytest.fixture(scope='module')
def edge_cases():
    return B.edge_cases()


@pytest.mark.parametrize('name,i', EDGES)
def test_edges(tmp_path, edge_cases, name, i):
    from mcaller_amd.device import get_device
    text, options = edge_cases[name]
    opts = options[i]
    (want, said, n), (got, got_said, got_n), who = both(tmp_path, text, opts)
    assert who['by'] == 'device', who
    assert got == want and got_said == said and got_n == n
    st = get_device().bed_last_stats()
    assert st['n_lines'] == text.count(b'\n') + (len(text) > 0 and not text.endswith(b'\n'))
    assert st['n_entries'] == len(B.host_entries(text))
    if name == 'hot_site' and not opts['gff']:
        assert b'\t1e-05\t-\t100000\n' in got
    if name == 'fractions' and opts['thresh'] == 0.0 and not opts['gff'] and not opts['with_probs']:
        assert [l.split(b'\t')[4] for l in got.splitlines()] == [b'0.0', b'1.0', b'0.3333333333333333', b'0.6666666666666666', b'0.14285714285714285']
    if name.startswith('interleaved_vo') and opts['depth'] == 1:
        deep = [l for l in got.splitlines() if l.startswith(b'deep\t')][0]
        assert deep.split(b'\t')[-1].split(b',') == [b'0.%04d' % (j + 1) for j in range(int(deep.split(b'\t')[6]))]
        assert int(deep.split(b'\t')[6]) == (70000 if name.endswith('wide') else 5000)


def test_the_text_entry_point_equals_the_file_entry_point(tmp_path, edge_cases):
    from mcaller_amd.device import get_device
    text, options = edge_cases['tile_edge_+0']
    src = tmp_path / 'x.diffs.6'
    src.write_bytes(text)
    dev = get_device()
    for opts in options:
        kw = dict(min_depth=opts['depth'], mod_threshold=opts['thresh'], control=opts['control'], with_probs=opts['with_probs'], gff=opts['gff'])
        a = dev.bed_summarise(path=str(src), **kw)
        b = dev.bed_summarise(text=text, **kw)
        assert a == b and a[2] is None and a[1] > 0


@pytest.mark.parametrize('name', sorted(B.decline_cases()))
def test_declines(tmp_path, monkeypatch, name):
    """What the device refuses before it touches it: status 1 with the reason and the line, and through main --device the outcome
    of main without the flag -- the same bytes, or the same exception type."""
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    text, opts, reason, line = B.decline_cases()[name]
    dev = get_device()
    blob, n, why = dev.bed_summarise(text=text, min_depth=opts['depth'], mod_threshold=opts['thresh'], control=opts['control'],
                                     with_probs=opts['with_probs'], gff=opts['gff'])
    st = dev.bed_last_stats()
    assert blob is None and why and 'declines' in why
    assert (st['decline_reason'], st['decline_line']) == (reason, line)
    (tmp_path / 'case.eventalign.diffs.6').write_bytes(text)
    monkeypatch.chdir(tmp_path)
    argv = ['-f', 'case.eventalign.diffs.6', '-d', str(opts['depth']), '-t', str(opts['thresh'])] + (['--vo'] if opts['with_probs'] else [])
    outcomes = []
    for extra in ([], ['--device']):
        out = tmp_path / 'case.methylation.summary.bed'
        if out.exists():
            out.unlink()
        make_bed.last_summary = None
        try:
            said = _main(argv + extra)
            outcomes.append((out.read_bytes(), said.splitlines()[1:]))
        except Exception as e:                                       # noqa
            outcomes.append(type(e))
    assert outcomes[0] == outcomes[1]
    if not isinstance(outcomes[1], type):
        assert make_bed.last_summary['by'] == 'host' and 'declines' in make_bed.last_summary['reason']


def test_a_table_that_is_too_small_declines(tmp_path, monkeypatch):
    from mcaller_amd.device import get_device
    text, opts = B.random_case(11)
    assert len(B.host_entries(text)) > 2
    monkeypatch.setenv('MCALLER_BED_TABLE_SLOTS', '4')
    (want, said, n), (got, got_said, got_n), who = both(tmp_path, text, opts)
    st = get_device().bed_last_stats()
    assert st['decline_reason'] == 9 and st['table_slots'] == 4
    assert who['by'] == 'host' and 'slots' in who['reason'] and got == want and got_said == said


def test_product_bed_vo_uses_the_device_summary(tmp_path, monkeypatch):
    """mCaller --bed --bed_vo on the committed testdata: the BED's lists come from the device summary; MCALLER_BED_DEVICE=0 (the
    Python pass) writes the same bytes."""
    from mcaller_amd import mCaller, make_bed
    (tmp_path / 'td').mkdir()
    td = H.testdata_paths(str(tmp_path / 'td'))
    model = os.path.join(H.MODELS, 'r95_twobase_model_NN_6_m6A.npz')
    beds = []
    for off in (False, True):
        d = tmp_path / ('run%d' % off)
        d.mkdir()
        tsv = str(d / 'masonread1.eventalign.tsv')
        shutil.copy(td['tsv'], tsv)
        if off:
            monkeypatch.setenv('MCALLER_BED_DEVICE', '0')
        make_bed.last_summary = None
        with contextlib.redirect_stdout(io.StringIO()):
            mCaller.main(['-m', 'GATC', '-r', td['fasta'], '-e', tsv, '-f', td['fastq'], '-d', model, '--bed', '--bed_vo',
                          '--bed_min_depth', '1'])
        beds.append(open(str(d / 'masonread1.methylation.summary.bed'), 'rb').read())
        if off:
            assert make_bed.last_summary is None
        else:
            assert make_bed.last_summary['by'] == 'device', make_bed.last_summary
    assert beds[0] == beds[1] and beds[0].count(b'\n') > 0
    assert beds[0] == open(os.path.join(H.GOLDEN, 'ref_outputs', 'motif_GATC.vo.bed'), 'rb').read()
