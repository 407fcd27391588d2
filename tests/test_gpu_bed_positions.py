"""make_bed -p on the GPU (mcaller_amd/csrc/bed/: the position set, the value matrix, the per-site t-tests of mc_tstat.h) writes
the bytes of make_bed's host code with SciPy -- itself pinned to the reference's outputs by tests/test_make_bed.py -- or declines
the file.  Every assertion on bytes comes with one on WHO made them (make_bed.last_summary).  tests/test_tstat.py shows on the CPU
that the same arithmetic meets no rounding tie on the files used here."""
import contextlib
import io
import json
import os
import shutil
import warnings

import numpy as np
import pytest

from tests import bedpos_files as P
from tests import helpers as H
from tests import tstat_grid as G

pytestmark = pytest.mark.gpu


def _main(argv):
    from mcaller_amd import make_bed
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        make_bed.main(argv)
    return buf.getvalue()


def test_device_tstat_against_the_host_build_on_the_grid():
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    df, t, scipy_l = G.grid()
    n, mean, var = G.triples(df, t)
    st, got_t, got_l = get_device().tstat(n, mean, var)
    host = np.array([_lib.tstat(a, b, c) for a, b, c in zip(n, mean, var)])
    assert (st == 0).all() and (host[:, 0] == 0).all()
    assert (got_t == host[:, 1]).all()
    err = G.relative_error(got_l, host[:, 2])
    print('device against host build, largest error / max(1, |log10 p|): %.3g; against SciPy: %.3g' % (err.max(), G.relative_error(got_l, scipy_l).max()))
    assert err.max() <= G.FN_BOUND / 8
    st, got_t, got_l = get_device().tstat([1, 3, 3, 100, 3], [2.0, 2.0, float('inf'), 1e6, 0.0], [0.0, 0.0, 1.0, 1e-12, 1.0])
    assert list(st) == [1, 2, 2, 4, 0] and np.isnan(got_t[:3]).all() and (got_t[4], got_l[4]) == (0.0, 0.0)
    assert get_device().tstat([], [], [])[0].shape == (0,)


def _golden_run(tmp_path, monkeypatch, tag, extra=()):
    from mcaller_amd import make_bed
    case = json.load(open(os.path.join(H.GOLDEN, 'bed_cases', 'manifest.json')))['cases'][tag]
    shutil.copy(os.path.join(H.GOLDEN, 'bed_cases', 'multi.eventalign.diffs.6'), str(tmp_path / 'multi.eventalign.diffs.6'))
    args = [{'<POS>': os.path.join(H.GOLDEN, 'bed_cases', 'bed_positions.txt')}.get(a, a) for a in case['args']]
    monkeypatch.chdir(tmp_path)
    make_bed.last_summary = None
    said = _main(['-f', 'multi.eventalign.diffs.6'] + args + list(extra) + ['--device'])
    return case, said, open(str(tmp_path / case['stem']), 'rb').read()


@pytest.mark.parametrize('tag', ['positions', 'positions_vo'])
def test_reference_goldens_on_the_device(tmp_path, monkeypatch, tag):
    from mcaller_amd import make_bed
    monkeypatch.setenv('MCALLER_BED_POSITIONS_DEVICE', '1')
    case, said, got = _golden_run(tmp_path, monkeypatch, tag)
    want = open(os.path.join(H.GOLDEN, 'bed_cases', case['output']), 'rb').read()
    assert got == want and want.count(b'\tnan\tnan') == 5
    assert 'loci found' not in said
    assert make_bed.last_summary == dict(by='device', reason=None, n_sites=want.count(b'\n'))


def test_the_knob_and_the_options_that_stay_with_the_host(tmp_path, monkeypatch):
    from mcaller_amd import make_bed
    monkeypatch.delenv('MCALLER_BED_POSITIONS_DEVICE', raising=False)
    _golden_run(tmp_path, monkeypatch, 'positions')
    assert make_bed.last_summary['by'] == 'host' and make_bed.last_summary['reason'] == 'out of scope on the device: -p'
    monkeypatch.setenv('MCALLER_BED_POSITIONS_DEVICE', '1')
    _, _, with_knob = _golden_run(tmp_path, monkeypatch, 'positions', extra=['--gff', '--vo'])
    assert make_bed.last_summary['by'] == 'host' and make_bed.last_summary['reason'] == 'out of scope on the device: -p'
    span = json.load(open(os.path.join(H.GOLDEN, 'testdata', 'rebuilt_fasta_span.json')))
    fasta = str(tmp_path / 'ref.fasta')
    open(fasta, 'w').write('>%s\n%s\n' % (span['contig'], 'N' * span['span_start'] + span['span'] + 'N' * 200))
    _golden_run(tmp_path, monkeypatch, 'positions', extra=['--ref', fasta])
    assert make_bed.last_summary['by'] == 'host' and 'out of scope' in make_bed.last_summary['reason']


def both(tmp_path, text, ptext, opts):
    """-> (host bytes, stdout, n), (device bytes, stdout, n), last_summary of one text, positions text and option set."""
    from mcaller_amd import make_bed
    src, pos = tmp_path / 'case.diffs.6', tmp_path / 'case.positions'
    src.write_bytes(text)
    pos.write_bytes(ptext)
    out = []
    for fn in (make_bed.summarise_diffs, make_bed.summarise_diffs_device):
        dst = tmp_path / ('out.' + fn.__name__)
        buf = io.StringIO()
        make_bed.last_summary = None
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            n = fn(str(src), str(dst), 15, 0.5, positions=str(pos), **opts)
        out.append((dst.read_bytes(), buf.getvalue(), n))
    return out[0], out[1], make_bed.last_summary


@pytest.fixture(scope='module')
def edge_cases():
    return P.edge_cases()


EDGES = [(name, i) for name, (_, _, options) in sorted(P.edge_cases().items()) for i in range(len(options))]


@pytest.mark.parametrize('name,i', EDGES)
def test_edges(tmp_path, edge_cases, name, i):
    from mcaller_amd.device import get_device
    text, ptext, options = edge_cases[name]
    opts = options[i]
    (want, said, n), (got, got_said, got_n), who = both(tmp_path, text, ptext, opts)
    assert who == dict(by='device', reason=None, n_sites=n), who
    assert got == want and got_said == said == '' and got_n == n
    st = get_device().bed_last_stats()
    assert st['n_sites'] == st['n_entries'] == n == want.count(b'\n')
    if name in ('positions_empty', 'positions_short_lines', 'nothing_wanted'):
        assert want == b'' and st['n_counted'] == 0
    if name == 'minus_zero':
        assert got.split(b'\t')[7] == b'-0.0'
    if name == 'depths' and not opts['gff']:
        assert [l.split(b'\t')[6] for l in got.splitlines()] == [b'1', b'2', b'3', b'32', b'33', b'257', b'64', b'65']
        assert got.splitlines()[0].split(b'\t')[7:9] == [b'nan', b'nan']
    if name == 'interleaved_5000':
        assert b'\t5000\t' in got.splitlines()[0] and n == 101
    if name == 'unwanted_unparseable':
        assert n == 3


def test_the_text_entry_point_equals_the_file_entry_point(tmp_path, edge_cases):
    from mcaller_amd.device import get_device
    text, ptext, options = edge_cases['depths']
    (tmp_path / 'x.diffs.6').write_bytes(text)
    (tmp_path / 'x.pos').write_bytes(ptext)
    dev = get_device()
    for opts in options:
        a = dev.bed_summarise(path=str(tmp_path / 'x.diffs.6'), positions_path=str(tmp_path / 'x.pos'), **opts)
        b = dev.bed_summarise(text=text, positions_text=ptext, **opts)
        assert a == b and a[2] is None and a[1] == 8


DECLINES = P.decline_cases()


@pytest.mark.parametrize('name', sorted(DECLINES))
def test_declines(tmp_path, name):
    """Every new reason with its code and line; through summarise_diffs_device the file is then the host's, or the host's error."""
    from mcaller_amd import make_bed
    from mcaller_amd.device import get_device
    text, ptext, opts, reason, line = DECLINES[name]
    dev = get_device()
    blob, n, why = dev.bed_summarise(text=text, positions_text=ptext, **opts)
    st = dev.bed_last_stats()
    assert blob is None and why and 'declines' in why
    assert (st['decline_reason'], st['decline_line']) == (reason, line)
    outcomes = []
    src, pos = tmp_path / 'case.diffs.6', tmp_path / 'case.positions'
    src.write_bytes(text)
    pos.write_bytes(ptext)
    for fn in (make_bed.summarise_diffs, make_bed.summarise_diffs_device):
        make_bed.last_summary = None
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                fn(str(src), str(tmp_path / 'out'), 15, 0.5, positions=str(pos), **opts)
            outcomes.append((tmp_path / 'out').read_bytes())
        except Exception as e:                                       # noqa
            outcomes.append(type(e))
    assert outcomes[0] == outcomes[1]
    if not isinstance(outcomes[1], type):
        assert make_bed.last_summary['by'] == 'host' and 'declines' in make_bed.last_summary['reason']


@pytest.fixture(scope='module')
def host_results(tmp_path_factory):
    """The host function's bytes for every random file, made once (both hash-mask runs compare with them)."""
    from mcaller_amd import make_bed
    d = tmp_path_factory.mktemp('bedpos_random')
    res = {}
    for seed in range(P.SEED_BASE, P.SEED_BASE + P.N_RANDOM):
        text, ptext, opts = P.random_case(seed)
        src, pos, dst = d / ('r%d.diffs.6' % seed), d / ('r%d.positions' % seed), d / 'host.out'
        src.write_bytes(text)
        pos.write_bytes(ptext)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            n = make_bed.summarise_diffs(str(src), str(dst), 15, 0.5, positions=str(pos), **opts)
        res[seed] = (str(src), str(pos), opts, dst.read_bytes(), n)
    return d, res


@pytest.mark.parametrize('mask', [None, 'f'])
def test_random_files(host_results, monkeypatch, mask):
    """200 generated files of 1-400 rows with a positions file each: the device's bytes are the host function's and the device
    declines none.  MCALLER_BED_HASH_MASK=f leaves 16 hash values for the entries AND for the position tuples: the byte
    comparisons decide."""
    from mcaller_amd import make_bed
    if mask:
        monkeypatch.setenv('MCALLER_BED_HASH_MASK', mask)
    else:
        monkeypatch.delenv('MCALLER_BED_HASH_MASK', raising=False)
    d, res = host_results
    n_rows = 0
    for seed, (src, pos, opts, want, n) in res.items():
        dst = d / 'device.out'
        got_n = make_bed.summarise_diffs_device(src, str(dst), 15, 0.5, positions=pos, quiet=True, **opts)
        assert make_bed.last_summary == dict(by='device', reason=None, n_sites=n), (seed, make_bed.last_summary)
        assert dst.read_bytes() == want and got_n == n, (seed, opts)
        n_rows += n
    assert n_rows > 400
