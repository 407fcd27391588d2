"""phase_reads on the GPU (mcaller_amd/csrc/compare/mc_readphase.inc, csrc/mc_pairphase.h; Device.reads_phase,
phase_reads.phase_reads_device) against the host statement: the device's bytes equal the host's -- rows, reads and bed, text to text
and file to file, with `reason is None` on every case that is not a decline; every decline with its reason and line and the host's
output behind it.  tests/test_phase_cases.py holds the cases to what they claim and shows, on the host builds, that none of those the
device is expected to make carries a Fisher status bit, a q-value tie or an nlp tie."""
import pytest

from mcaller_amd import _lib
from mcaller_amd import phase_reads as P
from tests import phase_cases as K

pytestmark = pytest.mark.gpu

WAVE, GROUP, MAX_DEPTH = _lib.PHASE_WAVE_ROWS, _lib.PHASE_GROUP_ROWS, _lib.PHASE_MAX_DEPTH


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def device_makes_it(dev, tmp_path, text, opt, fdr=False, threshold=2.0, what='', files=True):
    """The device's three outputs equal the host statement's, from the text and from the file; -> (rows, reads, bed, figures)."""
    p = K.write(tmp_path, text)
    want, want_reads, want_bed, fig = P._rows(p, fdr=fdr, threshold=threshold, want_reads=True, want_bed=True, **opt)
    got = dev.reads_phase(text=text, fdr=fdr, threshold=threshold, **opt)
    assert got[6] is None, (what, got[6])
    assert got[:6] == (want, want_reads, want_bed, fig['n_pairs'], fig['n_reads'], fig['n_linked']), what
    if files:
        out, reads, bed = (str(tmp_path / n) for n in ('out.tsv', 'out.reads', 'linked.bed'))
        assert P.phase_reads_device(p, out=out, fdr=fdr, reads=reads, linked_bed=bed, threshold=threshold, **opt) == fig['n_pairs']
        assert P.last_phase == dict(by='device', reason=None, **dict(fig, n_duplicates=0)), (what, P.last_phase)
        assert (open(out, 'rb').read(), open(reads, 'rb').read(), open(bed, 'rb').read()) == (want, want_reads, want_bed), what
    return want, want_reads, want_bed, fig


def host_does_it(dev, tmp_path, text, opt, reason, line, fdr=False):
    """The device declines with the reason and line, and the host statement's output stands behind it."""
    p = K.write(tmp_path, text)
    want, want_reads, want_bed, fig = P._rows(p, fdr=fdr, threshold=1.0, want_reads=True, want_bed=True, **opt)
    out, reads, bed = (str(tmp_path / n) for n in ('out.tsv', 'out.reads', 'linked.bed'))
    assert P.phase_reads_device(p, out=out, fdr=fdr, reads=reads, linked_bed=bed, threshold=1.0, **opt) == fig['n_pairs']
    assert P.last_phase['by'] == 'host' and P.last_phase['reason'] and dict(P.last_phase, by=0, reason=0) == dict(fig, by=0, reason=0), P.last_phase
    assert (open(out, 'rb').read(), open(reads, 'rb').read(), open(bed, 'rb').read()) == (want, want_reads, want_bed)
    st = dev.reads_phase_last_stats()
    assert st['decline_reason'] == _lib.CMP_DECLINE[reason] and (line is None or st['decline_line'] == line), st
    return st


@pytest.mark.parametrize('fdr', [False, True])
@pytest.mark.parametrize('name', sorted(K.DEVICE_CASES))
def test_device_equals_host(dev, tmp_path, name, fdr):
    text, opt, claims = K.DEVICE_CASES[name]()
    rows, _, _, fig = device_makes_it(dev, tmp_path, text, opt, fdr=fdr, threshold=0.3, what=name)
    assert fig['n_pairs'] > 0 and dev.reads_phase_last_stats()['window'] == claims['window']


def test_stats_of_the_read_lengths(dev, tmp_path):
    """Reads of 1, 2, 63, 64 and 65 rows and of the workgroup's cap: who ordered them, W, the counters, the pair instances."""
    text, opt, claims = K.case_read_lengths()
    _, _, _, fig = device_makes_it(dev, tmp_path, text, opt, what='lengths', files=False)
    st = dev.reads_phase_last_stats()
    n_wave = 8 + sum(1 for n in claims['lengths'] if n <= WAVE)
    assert (st['n_read_keys'], st['n_reads_wave'], st['n_reads_group'], st['longest_read']) == (fig['n_reads'], n_wave, 2, GROUP), st
    assert (st['n_sites'], st['window'], st['n_counters'], st['n_pairs'], st['n_reads']) == (GROUP, 3, 3 * GROUP, fig['n_pairs'], fig['n_reads']), st
    # a read of n rows one base apart makes (n - 1) + (n - 2) + (n - 3) pair instances under max_dist 3
    assert st['n_instances'] == sum(sum(max(n - k, 0) for k in (1, 2, 3)) for n in tuple(claims['lengths']) + (40,) * 8), st
    assert st['decline_reason'] == 0 and st['decline_line'] == -1


def test_a_read_beyond_the_cap_declines(dev, tmp_path):
    text, opt, _ = K.case_read_lengths(lengths=(5, GROUP + 1))
    first = text.decode().splitlines().index(next(l for l in text.decode().splitlines() if '\tlen%d\t' % (GROUP + 1) in l))
    st = host_does_it(dev, tmp_path, text, opt, 'read_rows', first)
    assert st['longest_read'] == GROUP + 1 and '2048 rows' in P.last_phase['reason']


def test_a_threshold_between_the_rows(dev, tmp_path):
    """A threshold taken from the rows themselves: pairs on both sides of it, with p and with q."""
    text, opt, _ = K.case_shuffled()
    for fdr in (False, True):
        rows = [r.split('\t') for r in P._rows(K.write(tmp_path, text), fdr=fdr, **opt)[0].decode().splitlines()]
        values = sorted(float(r[-1]) for r in rows)
        distinct = sorted(set(values))
        t = distinct[len(distinct) // 2]                                # (most pairs of the file are unlinked and print 0.0)
        assert len(distinct) > 2 and values[0] < t <= values[-1]
        _, _, bed, fig = device_makes_it(dev, tmp_path, text, opt, fdr=fdr, threshold=t, what='threshold %r' % t)
        links = sum(int(l.split('\t')[4]) for l in bed.decode().splitlines())
        assert 0 < fig['n_linked'] <= 30 and links == 2 * sum(1 for v in values if v >= t) < 2 * len(values)


def test_hash_collisions_in_both_tables(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', 'f')
    text, opt, _ = K.case_strands_and_chroms()
    device_makes_it(dev, tmp_path, text, opt, fdr=True, threshold=1.0, what='sixteen chains')
    st = dev.reads_phase_last_stats()
    assert st['longest_probe'] > 2 and st['longest_read_probe'] > 2, st


def test_small_stages(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_TEXT_STAGE_BYTES', '1000')
    for newline in (True, False):
        text, opt, _ = K.case_shuffled(newline=newline)
        assert len(text) > 10000
        device_makes_it(dev, tmp_path, text, opt, fdr=True, threshold=1.0, what=newline)


def test_the_depth_cap(dev, tmp_path):
    """A site of 65535 rows is made (no 16-bit field can carry), one of 65536 is DEPTH at the site's first line."""
    text, opt, _ = K.case_depth_cap(MAX_DEPTH)
    rows, _, _, fig = device_makes_it(dev, tmp_path, text, opt, what='65535', files=False)
    assert fig['n_pairs'] == 1 and rows.split(b'\t')[4] == b'24' and dev.reads_phase_last_stats()['deepest_site'] == MAX_DEPTH
    text, opt, _ = K.case_depth_cap(MAX_DEPTH + 1)
    host_does_it(dev, tmp_path, text, opt, 'depth', 0)


def test_a_duplicate_call_declines(dev, tmp_path):
    """A read with a second row at a position: the later line is named, the host's first-wins rule does the file."""
    text, opt, _ = K.case_shuffled()
    lines = text.decode().splitlines(True)
    f = lines[100].rstrip('\n').split('\t')
    f[6] = 'A' if f[6] == 'm6A' else 'm6A'                             # the later row says the opposite: the first wins
    lines.insert(300, '\t'.join(f) + '\n')
    st = host_does_it(dev, tmp_path, ''.join(lines).encode(), opt, 'duplicate', 300)
    assert P.last_phase['n_duplicates'] == 1


def test_memory_and_table_declines_then_clean_calls(dev, tmp_path, monkeypatch):
    """The counters beside a budget that holds the text and its tables; a key table that holds the sites and not the reads; then the
    same context makes the cases again: nothing of a declined call is left (the suite runs with poisoned allocations where
    MCALLER_POISON is set)."""
    text, opt, claims = K.case_counter_memory()
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', str(2 << 20))
    st = host_does_it(dev, tmp_path, text, opt, 'memory', -1)
    assert (st['window'], st['n_counters']) == (claims['window'], 300 * claims['window']) and 'counters' in P.last_phase['reason']
    monkeypatch.delenv('MCALLER_CMP_DEVICE_BYTES')
    device_makes_it(dev, tmp_path, text, opt, fdr=True, threshold=1.0, what='the counters fit')
    many, many_opt, _ = K.case_many_reads()
    monkeypatch.setenv('MCALLER_CMP_TABLE_SLOTS', '64')
    st = host_does_it(dev, tmp_path, many, many_opt, 'table', None)       # (which read's line meets the full table depends on arrival)
    assert st['n_sites'] == 4 and st['read_table_slots'] == 64
    monkeypatch.delenv('MCALLER_CMP_TABLE_SLOTS')
    device_makes_it(dev, tmp_path, many, many_opt, what='the reads fit')
    first = dev.reads_phase(text=text, threshold=1.0, **opt)
    dev.reads_phase_release()
    assert dev.reads_phase(text=text, threshold=1.0, **opt) == first and first[6] is None
    assert dev.reads_phase(text=b'', **opt) == (b'', b'', b'', 0, 0, 0, None)


def test_a_decline_then_clean_calls_with_poisoned_allocations(tmp_path):
    """A process of its own: the library reads MCALLER_POISON once.  Every fresh device block is filled with 0xAB, so a counter, a
    link count or a length that a kernel reads before anything wrote it shows up as a mismatch."""
    import os
    import subprocess
    import sys
    from tests import helpers as H
    env = dict(os.environ, MCALLER_POISON='1', PYTHONPATH=H.REPO)
    done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_phase_worker.py'), str(tmp_path)], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0 and b'phase ok' in done.stdout, done.stdout.decode('utf-8', 'replace')[-3000:]
