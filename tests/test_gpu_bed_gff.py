"""make_bed --gff --vo and --ref on the GPU (mcaller_amd/csrc/bed/mc_gffstats.inc, mc_fastactx.inc; MCALLER_BED_GFF_DEVICE=1) write
the bytes of make_bed's host code -- itself pinned to the reference's outputs by tests/test_make_bed.py -- or decline the file.  Every
assertion on bytes comes with one on WHO made them (make_bed.last_summary).  tests/test_gff_stats.py shows on the CPU that the same
arithmetic is NumPy's and that the random files used here meet no decline."""
import contextlib
import io
import json
import os
import shutil
import warnings

import numpy as np
import pytest

from tests import gffstats_files as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

REASONS = {'gff_vo_d2': '--gff with --vo', 'ref_d2': '--ref'}


def _main(argv):
    from mcaller_amd import make_bed
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        make_bed.main(argv)
    return buf.getvalue()


def _span_fasta(tmp_path):
    span = json.load(open(os.path.join(H.GOLDEN, 'testdata', 'rebuilt_fasta_span.json')))
    fasta = str(tmp_path / 'ref.fasta')
    open(fasta, 'w').write('>%s\n%s\n' % (span['contig'], 'N' * span['span_start'] + span['span'] + 'N' * 200))
    return fasta


def _golden_run(tmp_path, monkeypatch, tag):
    from mcaller_amd import make_bed
    case = json.load(open(os.path.join(H.GOLDEN, 'bed_cases', 'manifest.json')))['cases'][tag]
    shutil.copy(os.path.join(H.GOLDEN, 'bed_cases', 'multi.eventalign.diffs.6'), str(tmp_path / 'multi.eventalign.diffs.6'))
    args = [{'<REF>': _span_fasta(tmp_path)}.get(a, a) for a in case['args']]
    monkeypatch.chdir(tmp_path)
    make_bed.last_summary = None
    said = _main(['-f', 'multi.eventalign.diffs.6'] + args + ['--device'])
    want = open(os.path.join(H.GOLDEN, 'bed_cases', case['output']), 'rb').read()
    assert open(str(tmp_path / case['stem']), 'rb').read() == want
    assert case['summary_line'] in said
    return int(case['summary_line'].split()[0])


@pytest.mark.parametrize('tag', sorted(REASONS))
def test_reference_goldens_with_and_without_the_knob(tmp_path, monkeypatch, tag):
    from mcaller_amd import make_bed
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    n = _golden_run(tmp_path, monkeypatch, tag)
    assert make_bed.last_summary == dict(by='device', reason=None, n_sites=n)
    monkeypatch.delenv('MCALLER_BED_GFF_DEVICE')
    _golden_run(tmp_path, monkeypatch, tag)
    assert make_bed.last_summary['by'] == 'host' and make_bed.last_summary['reason'] == 'out of scope on the device: ' + REASONS[tag]


def test_the_golden_with_ref_and_gff_and_vo(tmp_path, monkeypatch):
    """--ref --gff and --ref --gff --vo of the committed file: the host function's bytes, contexts from the FASTA in them."""
    fasta = _span_fasta(tmp_path)
    src = os.path.join(H.GOLDEN, 'bed_cases', 'multi.eventalign.diffs.6')
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    for vo in (False, True):
        (want, said, n), (got, got_said, got_n), who = both(tmp_path, open(src, 'rb').read(), dict(depth=2, thresh=0.5, gff=True, with_probs=vo), fasta=open(fasta, 'rb').read())
        assert who == dict(by='device', reason=None, n_sites=n) and got == want and got_said == said and n > 0
        assert (b';fracLow=' in got) == vo


# ---- the arithmetic on the device ---------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def test_device_site_stats_equal_the_host_build():
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    arrays = [F.seeded_array(n) for n in F.N_LIST] + [F.equal_array(n, v) for n in (2, 9, 129, 8193) for v in (0.5, 0.62)] + [[0.3], [-0.5, 1e-9, 2.5e6]]
    frac = [(i % 4) / 3.0 for i in range(len(arrays))]
    st, out = get_device().gff_site_stats(arrays, frac)
    for i, p in enumerate(arrays):
        h_st, lo, up, qv = _lib.gff_site_stats(p, frac[i])
        m_st, mean, var, se = _lib.gff_site_moments(p)
        assert h_st == st[i] and m_st == 0, (len(p), h_st, st[i])
        assert _same(out[i], [lo, up, qv, mean, var, se]), (len(p), list(out[i]), [lo, up, qv, mean, var, se])
    assert st[F.N_LIST.index(1)] == 1 and np.isnan(out[F.N_LIST.index(1), :2]).all()


def test_device_square_root_and_division():
    """10^5 variances -- uniform ones, and doubles within 2 ulp of a perfect square -- with their depths: sqrt(var) / sqrt(n) on the
    device is the correctly rounded one (NumPy's, and the host build's on a part)."""
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    var, n = F.variances()
    got = get_device().npsum_se(var, n)
    want = np.sqrt(np.array(var)) / np.sqrt(np.array(n))
    wrong = np.flatnonzero(got != want)
    print('sqrt(var) / sqrt(n): %d of %d differ' % (len(wrong), len(var)))
    assert len(wrong) == 0, [(var[i], n[i], got[i], want[i]) for i in wrong[:5]]
    assert all(got[i] == _lib.npsum_se(var[i], n[i]) for i in range(0, len(var), 50))


# ---- files ------------------------------------------------------------------------------------------------------------------------
def both(tmp_path, text, opts, fasta=None, monkeypatch=None):
    """-> (host bytes, stdout, n), (device bytes, stdout, n), last_summary of one text, option set and FASTA text (or None)."""
    from mcaller_amd import make_bed
    src, ref = tmp_path / 'case.diffs.6', tmp_path / 'case.fasta'
    src.write_bytes(text)
    if fasta is not None:
        ref.write_bytes(fasta)
    kw = dict(control=opts.get('control', False), with_probs=opts['with_probs'], gff=opts['gff'], ref=str(ref) if fasta is not None else None)
    out = []
    for fn in (make_bed.summarise_diffs, make_bed.summarise_diffs_device):
        dst = tmp_path / ('out.' + fn.__name__)
        buf = io.StringIO()
        make_bed.last_summary = None
        with contextlib.redirect_stdout(buf), warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            n = fn(str(src), str(dst), opts.get('depth', 1), opts.get('thresh', 0.5), **kw)
        out.append((dst.read_bytes(), buf.getvalue(), n))
    return out[0], out[1], make_bed.last_summary


@pytest.fixture(scope='module')
def depth_text():
    return F.depth_file()


@pytest.mark.parametrize('i', range(len(F.DEPTH_OPTIONS)))
def test_entries_of_every_depth(tmp_path, monkeypatch, depth_text, i):
    """One entry per depth at which NumPy's order of additions changes, their rows interleaved: -d 1 with -t 0.0, and --control."""
    from mcaller_amd.device import get_device
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    opts = dict(F.DEPTH_OPTIONS[i], gff=True, with_probs=True)
    (want, said, n), (got, got_said, got_n), who = both(tmp_path, depth_text, opts)
    assert who == dict(by='device', reason=None, n_sites=n), who
    assert got == want and got_said == said and got_n == n
    depths = sorted(int(l.split(b'coverage=')[1].split(b';')[0]) for l in got.splitlines())
    if not opts['control']:
        assert depths == sorted(F.N_LIST) and got.count(b'fracLow=nan;fracUp=nan') == 1
    else:
        assert 5 <= len(depths) < len(F.N_LIST) and max(depths) > 8192
    assert get_device().bed_last_stats()['n_entries'] == len(F.N_LIST)


@pytest.fixture(scope='module')
def host_results(tmp_path_factory):
    """The host function's bytes for every random file, made once (both hash-mask runs compare with them)."""
    from mcaller_amd import make_bed
    d = tmp_path_factory.mktemp('bedgff_random')
    ref = d / 'random.fasta'
    ref.write_bytes(F.random_fasta())
    res = {}
    for seed in range(F.N_RANDOM):
        text, opts, with_ref = F.random_case(seed)
        src, dst = d / ('r%d.diffs.6' % seed), d / 'host.out'
        src.write_bytes(text)
        kw = dict(control=opts['control'], with_probs=True, gff=True, ref=str(ref) if with_ref else None)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            n = make_bed.summarise_diffs(str(src), str(dst), opts['depth'], opts['thresh'], **kw)
        res[seed] = (str(src), opts, kw, dst.read_bytes(), buf.getvalue(), n)
    return d, res


@pytest.mark.parametrize('mask', [None, 'f'])
def test_random_files(host_results, monkeypatch, mask):
    """300 generated files of 1-400 rows, --gff --vo with and without --control and --ref: the device's bytes and summary line are
    the host function's and the device declines none.  MCALLER_BED_HASH_MASK=f leaves 16 hash values for the entries AND for the
    FASTA's ids: the byte comparisons decide."""
    from mcaller_amd import make_bed
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    if mask:
        monkeypatch.setenv('MCALLER_BED_HASH_MASK', mask)
    else:
        monkeypatch.delenv('MCALLER_BED_HASH_MASK', raising=False)
    d, res = host_results
    n_sites = n_ref = 0
    for seed, (src, opts, kw, want, said, n) in res.items():
        dst = d / 'device.out'
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got_n = make_bed.summarise_diffs_device(src, str(dst), opts['depth'], opts['thresh'], **kw)
        assert make_bed.last_summary == dict(by='device', reason=None, n_sites=n), (seed, make_bed.last_summary)
        assert dst.read_bytes() == want and buf.getvalue() == said and got_n == n, (seed, opts)
        n_sites += n
        n_ref += kw['ref'] is not None
    assert n_sites > 1000 and 100 < n_ref < 200


REF_CASES = F.ref_cases()


@pytest.mark.parametrize('name', sorted(REF_CASES))
def test_ref_edges(tmp_path, monkeypatch, name):
    """The slice rule at both ends of a contig and on contigs shorter than a window, and the reader's rules, each with --gff, with
    --gff --vo and as the plain BED (which keeps the rows' contexts)."""
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    fasta, text = REF_CASES[name]
    for opts in F.REF_OPTIONS:
        (want, said, n), (got, got_said, got_n), who = both(tmp_path, text, opts, fasta=fasta)
        assert who == dict(by='device', reason=None, n_sites=n), (opts, who)
        assert got == want and got_said == said and got_n == n and n > 0, opts
        if opts['gff']:
            contexts = [l.split(b'context=')[1].split(b';')[0] for l in got.splitlines()]
            assert max(len(c) for c in contexts) == 41 and b'AMA' not in contexts
            assert b'' in contexts
        else:
            assert all(l.split(b'\t')[3] == b'AMA' for l in got.splitlines())


def test_repeated_id_in_one_probe_chain(tmp_path, monkeypatch):
    """Twelve records in one probe chain (MCALLER_BED_HASH_MASK=f, ids chosen for it), `ctg` the first, the sixth and the last of them
    with three sequences: the last record wins, wherever in the chain the id stands."""
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    monkeypatch.setenv('MCALLER_BED_HASH_MASK', 'f')
    fasta, text = F.chained_ids_case()
    for opts in F.REF_OPTIONS[:2]:
        (want, said, n), (got, got_said, got_n), who = both(tmp_path, text, opts, fasta=fasta)
        assert who == dict(by='device', reason=None, n_sites=n), (opts, who)
        assert got == want and got_said == said and got_n == n and n > 0, opts
    assert F.SEQS['ctg'][:41].encode() in got and F._seq(F.REF_L, 9)[:41].encode() not in got


def test_the_text_entry_point_equals_the_file_entry_point(tmp_path):
    from mcaller_amd.device import get_device
    fasta, text = REF_CASES['repeated_id']
    (tmp_path / 'x.diffs.6').write_bytes(text)
    (tmp_path / 'x.fasta').write_bytes(fasta)
    dev = get_device()
    for kw in (dict(gff=True, with_probs=True), dict(gff=True), dict(gff=True, with_probs=True, control=True)):
        for ref in (False, True):
            a = dev.bed_summarise(path=str(tmp_path / 'x.diffs.6'), ref_path=str(tmp_path / 'x.fasta') if ref else None, min_depth=1, site_stats=True, **kw)
            b = dev.bed_summarise(text=text, ref_text=fasta if ref else None, min_depth=1, site_stats=True, **kw)
            assert a == b and a[2] is None and (a[1] > 0) != bool(kw.get('control'))      # (every entry's fraction is 0.5)
    blob, n, why = dev.bed_summarise(text=text, gff=True, with_probs=True)
    assert blob is None and dev.bed_last_stats()['decline_reason'] == 12          # (the older entry points decline --gff --vo as before)


def test_positions_with_gff_vo_and_with_ref(tmp_path, monkeypatch):
    """-p --gff --vo and -p --ref --gff on the committed files, both knobs set: the host function's bytes, from main --device."""
    from mcaller_amd import make_bed
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    monkeypatch.setenv('MCALLER_BED_POSITIONS_DEVICE', '1')
    fasta = _span_fasta(tmp_path)
    pos = os.path.join(H.GOLDEN, 'bed_cases', 'bed_positions.txt')
    shutil.copy(os.path.join(H.GOLDEN, 'bed_cases', 'multi.eventalign.diffs.6'), str(tmp_path / 'multi.eventalign.diffs.6'))
    monkeypatch.chdir(tmp_path)
    for extra in (['--gff', '--vo'], ['--ref', fasta, '--gff']):
        outs = []
        for device in ([], ['--device']):
            make_bed.last_summary = None
            _main(['-f', 'multi.eventalign.diffs.6', '-p', pos] + extra + device)
            outs.append(open('multi.methylation.positions.summary.gff', 'rb').read())
            os.remove('multi.methylation.positions.summary.gff')
        assert outs[0] == outs[1] and outs[0].count(b'\n') > 5
        assert make_bed.last_summary == dict(by='device', reason=None, n_sites=outs[0].count(b'\n'))
    monkeypatch.delenv('MCALLER_BED_POSITIONS_DEVICE')
    _main(['-f', 'multi.eventalign.diffs.6', '-p', pos, '--gff', '--vo', '--device'])
    assert make_bed.last_summary['by'] == 'host' and make_bed.last_summary['reason'] == 'out of scope on the device: -p'


DECLINES = F.decline_cases()


@pytest.mark.parametrize('name', sorted(DECLINES))
def test_declines(tmp_path, monkeypatch, name):
    """Every new reason with its code and line; through main --device with the knob the outcome is that of main without --device:
    the same bytes, or the same exception type."""
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    text, fasta, opts, reason, line = DECLINES[name]
    dev = get_device()
    blob, n, why = dev.bed_summarise(text=text, ref_text=fasta, min_depth=1, site_stats=True, **opts)
    st = dev.bed_last_stats()
    assert blob is None and why and 'declines' in why
    assert (st['decline_reason'], st['decline_line']) == (reason, line)
    (tmp_path / 'case.eventalign.diffs.6').write_bytes(text)
    argv = ['-f', 'case.eventalign.diffs.6', '-d', '1', '--gff'] + (['--vo'] if opts['with_probs'] else [])
    if fasta is not None:
        (tmp_path / 'case.fasta').write_bytes(fasta)
        argv += ['--ref', 'case.fasta']
    monkeypatch.chdir(tmp_path)
    outcomes = []
    for extra in ([], ['--device']):
        out = tmp_path / 'case.methylation.summary.gff'
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
    assert isinstance(outcomes[0], type) == (name in ('nan_probability', 'unknown_contig', 'r_in_a_minus_window'))


def test_a_letter_outside_acgtnm_is_printed_on_plus(tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_BED_GFF_DEVICE', '1')
    text, fasta, opts, _, _ = DECLINES['r_in_a_minus_window']
    plus = b''.join(l + b'\n' for l in text.splitlines() if b'\t+\t' in l)
    (want, said, n), (got, got_said, got_n), who = both(tmp_path, plus, dict(opts, depth=1), fasta=fasta)
    assert who == dict(by='device', reason=None, n_sites=n) and got == want and n == 3
    assert all(b'R' in l.split(b'context=')[1].split(b';')[0] for l in got.splitlines())
