"""phase_reads on the GPU (mcaller_amd/csrc/compare/mc_readphase.inc, the kr_* kernels behind Device.reads_phase) on the cases of
tests/phase_edge_cases.py: reads of 65 .. 2048 rows whose rows arrive in no order (the LDS sort of kr_order<256, 2048>), duplicates
in a long read, at a site that is not kept and at a site only its duplicate keeps, count fields of 65530 and more (the packing of
kr_pairs, the unpacking of kr_finish and kr_put<0>), read keys and group keys equal in all but one field under three hash masks, group
head lines of 256 and 65536 (the upper passes of ph_sort_sites and their skip rule), --max_dist beyond 2^31, positions 0 and 999999999,
tables exactly at --min_reads and --min_margin, no pair at all, --threshold 0.0 and inf, Fisher values the device declines, and every
line decline.  Every served case: the device's bytes equal the host statement's, text to text and file to file, `reason is None`, and
the pair instances are the brute force's.  Every decline: its reason and line, and the host's output or error behind it.  That the
cases hold what they claim, and that the device has no reason to decline the served ones, is tests/test_phase_edge_cases.py's
business (CPU).  Runs on a real MI355X only."""
import pytest

from mcaller_amd import _lib
from mcaller_amd import phase_reads as P
from tests import phase_cases as K
from tests import phase_edge_cases as E
from tests.test_gpu_phase_reads import device_makes_it, host_does_it
from tests.test_phase_cases import window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def fields(rows):
    return [r.split('\t') for r in rows.decode().splitlines()]


def served(dev, tmp_path, name, threshold=0.3, files=True):
    """A case of E.SERVED through device_makes_it; the pair instances against the brute force's tables, W against the case's claim
    -> (rows, reads, bed, figures, stats, claims, kept sites)."""
    text, opt, claims = E.SERVED[name]()
    rows, reads, bed, fig = device_makes_it(dev, tmp_path, text, opt, fdr=name in E.FDR, threshold=threshold, what=name, files=files)
    st = dev.reads_phase_last_stats()
    kept, _, tables, _, _ = K.brute_tables(K.write(tmp_path, text), opt['depth'], opt['max_dist'])
    assert st['n_instances'] == sum(sum(t) for t in tables.values()), (name, st)
    assert (st['decline_reason'], st['decline_line'], st['n_sites']) == (0, -1, len(kept)), (name, st)
    if 'window' in claims:
        assert st['window'] == claims['window'], (name, st)
    return rows, reads, bed, fig, st, claims, kept


def test_long_reads_in_any_arrival(dev, tmp_path):
    """Seven reads of 65 .. 2048 rows, every row of the file at a random place and the file's lines in reverse: the workgroup's
    bitonic sort orders what it has never seen ordered, with a padded length that is a power of two (128, 2048) and is none."""
    outputs = []
    for name in ('long_shuffled', 'long_reversed'):
        rows, reads, bed, fig, st, claims, _ = served(dev, tmp_path, name)
        assert (st['n_reads_group'], st['n_reads_wave'], st['longest_read'], st['n_read_keys']) == (7, 8, E.GROUP, 15), st
        assert (st['n_sites'], st['n_lines'], st['n_counters']) == (E.GROUP - 1, 6762, 3 * (E.GROUP - 1)) and fig['n_pairs'] > 2000, st
        outputs.append(tuple(sorted(o.splitlines()) for o in (rows, reads, bed)))
    assert outputs[0] == outputs[1]                                     # the same lines, each file's in the order of its own first rows


@pytest.mark.parametrize('variant', ['one', 'two', 'unkept', 'by_duplicate'])
def test_duplicates_decline(dev, tmp_path, variant):
    """A copy in the 1025-row read (the workgroup's neighbour test), two of them (the smaller of the later lines), one at a site below
    -d, and one that alone brings its site to -d: the device counts rows, the host calls."""
    text, opt, claims = E.case_duplicate(variant)
    st = host_does_it(dev, tmp_path, text, opt, 'duplicate', claims['line'])
    assert P.last_phase['n_duplicates'] == claims['duplicates'] and 'two rows at one position' in P.last_phase['reason']
    if variant == 'by_duplicate':
        assert (P.last_phase['n_sites'], st['n_sites']) == (claims['host_sites'], claims['device_sites']) == (2, 3), st
    if variant in ('one', 'two'):
        assert st['longest_read'] == E.GROUP and st['n_reads_group'] == 7, st


def test_duplicates_without_a_kept_site_are_served(dev, tmp_path):
    rows, reads, bed, fig, st, _, kept = served(dev, tmp_path, 'duplicates_no_site')
    assert (rows, reads, bed) == (b'', b'', b'') and kept == [] and P.last_phase == dict(by='device', reason=None, n_sites=0, n_pairs=0, n_reads=0,
                                                                                         n_linked=0, n_duplicates=0)


@pytest.mark.parametrize('name', E.DEEP)
def test_count_fields_at_capacity(dev, tmp_path, name):
    """65535 reads over every site: between the three texts each of the four 16-bit fields of a counter holds 65530 or more."""
    rows, _, _, fig, st, claims, _ = served(dev, tmp_path, name, files=False)
    got = fields(rows)
    assert [tuple(int(v) for v in f[5:9]) for f in got] == claims['tables'] and all(f[4] == '65535' for f in got)
    assert fig['n_pairs'] == len(claims['tables']) and st['deepest_site'] == E.MAX_DEPTH and all(len(f) == 12 for f in got), st


@pytest.mark.parametrize('mask', [None, 'f', '0'])
def test_keys_equal_in_all_but_one_field(dev, tmp_path, monkeypatch, mask):
    if mask is not None:
        monkeypatch.setenv('MCALLER_CMP_HASH_MASK', mask)
    rows, reads, _, fig, st, claims, _ = served(dev, tmp_path, 'near_keys', threshold=1.0)
    assert (fig['n_pairs'], fig['n_reads'], st['n_keys'], st['n_read_keys']) == (claims['rows'], claims['reads'], claims['sites'], claims['reads']), st
    assert len({tuple(f[:4]) for f in fields(rows)}) == 63 and len({tuple(f[:3]) for f in fields(reads)}) == 84
    if mask == 'f':
        assert st['longest_probe'] > 2 and st['longest_read_probe'] > 2, st
    if mask == '0':                                                     # one chain: the bytes alone tell the keys apart
        assert st['longest_probe'] >= claims['sites'] and st['longest_read_probe'] >= claims['reads'], st


@pytest.mark.parametrize('form', ['full', '257', '65537'])
def test_group_lines_beyond_the_low_bytes(dev, tmp_path, form):
    """Head lines 0, 256 and 65536: the groups' sort keys differ above bit 40 alone, and 257 and 65537 lines are where ph_sort_sites
    begins to run the passes of those bits.  A wrong order leaves the bytes right only where W comes out wrong."""
    rows, _, _, fig, st, claims, kept = served(dev, tmp_path, 'group_lines_' + form)
    text, opt, _ = E.case_group_lines(form)
    assert st['window'] == window(E.unfilled(kept), opt['max_dist']) == claims['window'], st
    assert (st['n_lines'], st['n_sites']) == (claims['lines'], claims['sites']) and fig['n_pairs'] > 30, st


@pytest.mark.parametrize('name', ['max_dist_2^31-1', 'max_dist_2^31', 'max_dist_10^12'])
def test_max_dist_beyond_int32(dev, tmp_path, name):
    rows, _, _, fig, st, claims, _ = served(dev, tmp_path, name)
    assert st['window'] == 39 and st['n_counters'] == 40 * 39 and fig['n_pairs'] > 100, st


def test_positions_at_both_ends(dev, tmp_path):
    rows, _, bed, fig, _, _, _ = served(dev, tmp_path, 'far_positions', threshold=0.0)
    assert fig['n_pairs'] == 1 and fields(rows)[0][2:4] == ['0', '999999999']
    assert sorted(f[1:3] for f in fields(bed)) == [['0', '1'], ['999999999', '1000000000']]


def test_tables_at_the_option_edges(dev, tmp_path):
    """n = --min_reads and one below; a margin of --min_margin and one below; a margin of exactly 1 under --min_margin 1, of 0 never."""
    for name, want in (('table_edges_margin_2', [1000, 3000]), ('table_edges_margin_1', [1000, 3000, 4000])):
        rows = served(dev, tmp_path, name)[0]
        assert sorted(int(f[2]) for f in fields(rows)) == want
        assert {int(f[2]): tuple(int(v) for v in f[5:9]) for f in fields(rows)} == {a: E.EDGE_TABLES[a] for a in want}


def test_no_pair_among_kept_sites(dev, tmp_path):
    """--min_reads 2^40 with --fdr, the reads rows and the bed wanted: the q-values' column is not run, the reads rows stand."""
    rows, reads, bed, fig, st, claims, _ = served(dev, tmp_path, 'no_pair', threshold=0.0)
    assert (rows, bed) == (b'', b'') and reads.count(b'\n') == fig['n_reads'] == claims['reads'] and fig['n_pairs'] == st['n_pairs'] == 0, st


def test_thresholds_zero_and_inf(dev, tmp_path):
    text, opt, claims = E.case_near_keys()
    for fdr in (False, True):
        rows, _, bed, fig = device_makes_it(dev, tmp_path, text, opt, fdr=fdr, threshold=0.0, what='threshold 0.0')
        in_rows = {(f[0], f[1], pos) for f in fields(rows) for pos in f[2:4]}
        assert {(f[0], f[5], f[1]) for f in fields(bed)} == in_rows and fig['n_linked'] == claims['sites']
        assert sum(int(f[4]) for f in fields(bed)) == 2 * fig['n_pairs']
        _, _, bed, fig = device_makes_it(dev, tmp_path, text, opt, fdr=fdr, threshold=float('inf'), what='threshold inf')
        assert bed == b'' and fig['n_linked'] == 0 and fig['n_pairs'] == claims['rows']


def test_a_deep_linked_pair_beside_the_far_tail(dev, tmp_path):
    rows = served(dev, tmp_path, 'far_tail_served_alone')[0]
    assert fields(rows) == [['chr1', '+', '1000', '1005', '842', '420', '1', '1', '420', '0.995', '246.357']]


@pytest.mark.parametrize('which', ['one', 'two', 'deeper'])
def test_far_tail_declines(dev, tmp_path, which):
    """A deep, perfectly linked pair: log10 p below -250 (and, for 900 + 900 reads, the branch that has no finite value); the head
    line of site A is named, the smaller of two."""
    text, opt, claims = E.case_far_tail(which)
    host_does_it(dev, tmp_path, text, opt, 'far_tail', claims['line'])
    assert '-250' in P.last_phase['reason'] and 'line %d' % (claims['line'] + 1) in P.last_phase['reason'], P.last_phase
    assert P.last_phase['n_pairs'] == (3 if which == 'two' else 2)


def test_line_declines(dev, tmp_path):
    """Every line-level decline through reads_phase: reason and line; the host's output behind it, or its ValueError in its words."""
    for name, (text, opt, reason, line, error) in E.line_declines().items():
        if error is None:
            host_does_it(dev, tmp_path, text, opt, reason, line)
            continue
        p = K.write(tmp_path, text)
        with pytest.raises(ValueError) as host:
            P._rows(p, **opt)
        with pytest.raises(ValueError) as got:
            P.phase_reads_device(p, out=str(tmp_path / 'out.tsv'), **opt)
        assert str(got.value) == str(host.value) and error in str(got.value), (name, str(got.value))
        st = dev.reads_phase_last_stats()
        assert (st['decline_reason'], st['decline_line']) == (_lib.CMP_DECLINE[reason], line), (name, st)
    # behind them the device serves as before
    text, opt, _ = K.case_shuffled()
    device_makes_it(dev, tmp_path, text, opt, what='behind the declines')


def test_the_small_cases_with_poisoned_allocations(tmp_path):
    """A process of its own (the library reads MCALLER_POISON once): a decline, then the small served cases through one context."""
    import os
    import subprocess
    import sys
    from tests import helpers as H
    env = dict(os.environ, MCALLER_POISON='1', PYTHONPATH=H.REPO)
    done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_phase_edges_worker.py'), str(tmp_path)], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0 and b'phase edges ok' in done.stdout, done.stdout.decode('utf-8', 'replace')[-3000:]
