"""The site grouping (mcaller_amd/csrc/compare/mc_sitegroup.inc) and the two pipelines behind it -- compare_currents
(mc_curcompare.inc, the kc_rank_* kernels) and cluster_sites (mc_sitecluster.inc) -- on the cases of tests/sitegroup_cases.py: samples of
2 rows against 8190, one column and twenty-four, keys that differ at a field boundary only with a context per row, a hash mask of 0,
more than 1024 kept sites, a key over the depth cap that is not kept, numbers not spelled as repr() spells them, texts without a site,
and sites that one column declines.  Every served case: the device's bytes equal the host statement's, text to text and file to file,
`reason is None`, the device made the output, and the stats say which kernels ran.  Every decline: its reason, file and line, and the
host's output behind it.  That the cases hold what they claim, and that the device has no reason to decline the served ones, is
tests/test_sitegroup_cases.py's business (CPU).  Runs on a real MI355X only."""
import pytest

from mcaller_amd import compare_currents as CC
from tests import currents_cases as K
from tests import sitegroup_cases as G
from tests.test_gpu_cluster_sites import device_makes_it as cluster_device_makes_it
from tests.test_gpu_compare_currents import device_makes_it, host_does_it

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def fields(rows):
    return [r.split('\t') for r in rows.decode().splitlines()]


def test_unbalanced_samples_in_every_rank_kernel(dev, tmp_path):
    """2 rows against 62 .. 8190 and the other way round, one column: n1 is the rank kernels' index into the pooled vector."""
    native, control = G.unbalanced()
    rows, _, n = device_makes_it(dev, tmp_path, native, control, depth=2, fdr=True, what='unbalanced')
    st = dev.currents_compare_last_stats()
    assert (st['n_columns'], st['n_sites'], st['deepest_site']) == (1, 8, 8192) and n == 8, st
    assert (st['n_rank_small'], st['n_rank_large']) == (2, 6), st
    assert [(int(f[5]), int(f[6])) for f in fields(rows)] == G.UNBALANCED


def test_twenty_four_columns(dev, tmp_path):
    native, control = G.wide()
    p1, p2 = K.files(tmp_path, native, control)
    printed = sorted(set(float(f[-1]) for f in fields(CC.compare_rows(p1, p2, 3, True)[0])))
    assert len(printed) > 1
    rows, bed, n = device_makes_it(dev, tmp_path, native, control, depth=3, fdr=True, by='ks', threshold=printed[-1], what='wide')
    st = dev.currents_compare_last_stats()
    assert n == 12 and st['n_columns'] == 24 and st['n_rank_small'] + st['n_rank_large'] == 24 * st['n_sites'] == 24 * 12, st
    assert 0 < bed.count(b'\n') < n and all(len(f) == 7 + 24 + 8 for f in fields(rows))


@pytest.mark.parametrize('mask', [None, '0'])
def test_keys_at_field_boundaries_and_a_context_per_row(dev, tmp_path, monkeypatch, mask):
    """Keys whose bytes are equal once chrom and pos stand behind one another, pos 0 and 999999999, a context per row; under a hash
    mask of 0 every key hangs on one chain and the byte comparison alone tells them apart."""
    if mask is not None:
        monkeypatch.setenv('MCALLER_CMP_HASH_MASK', mask)
    native, control = G.keys_pair()
    ctx, order = G.first_contexts(native)
    rows, _, n = device_makes_it(dev, tmp_path, native, control, depth=3, what='keys, mask %s' % mask)
    st = dev.currents_compare_last_stats()
    got = fields(rows)
    assert n == 9 and [(f[0], int(f[1]), f[4]) for f in got] == [k for k in order if k in G.KEYS]
    assert len(set((f[0], f[1], f[4]) for f in got)) == 9
    assert all(f[3] == ctx[(f[0], int(f[1]), f[4])] for f in got)
    ends = {(f[0], f[1]): f[2] for f in got}
    assert ends[('c', '0')] == '1' and ends[('chr11', '0')] == '1' and ends[('c', '999999999')] == '1000000000'
    if mask == '0':
        assert st['longest_probe'] >= len(ctx) == 10, st
    # the same lines as one file: cluster_sites' grouping
    text = G.keys_text()
    ctx, order = G.first_contexts(text)
    rows, _, n = cluster_device_makes_it(dev, tmp_path, text, depth=2, what='keys, one file, mask %s' % mask)
    got = fields(rows)
    assert n == 10 and [(f[0], int(f[1]), f[4]) for f in got] == order and all(f[3] == ctx[(f[0], int(f[1]), f[4])] for f in got)
    if mask == '0':
        assert dev.sites_cluster_last_stats()['longest_probe'] >= 10


def test_more_kept_sites_than_a_scan_round(dev, tmp_path):
    """About 1170 kept sites among 1500 keys in two files shuffled as wholes: the scans over the sites' counts, row lengths and bed
    lengths, kn_combine and kn_size go beyond one 1024-wide round and one block."""
    native, control = G.many_pair()
    rows, bed, n = device_makes_it(dev, tmp_path, native, control, depth=2, fdr=True, by='t', threshold=0.0, what='many')
    st = dev.currents_compare_last_stats()
    assert n == st['n_sites'] == st['n_sig'] == bed.count(b'\n') > 1024 and st['n_columns'] == 1, st
    assert [f[:4] for f in fields(bed)] == [f[:4] for f in fields(rows)]


def test_more_kept_sites_than_a_scan_round_in_one_file(dev, tmp_path):
    text = G.many_text()
    rows, bed, n = cluster_device_makes_it(dev, tmp_path, text, depth=2, mixed=True, min_minor=0.0, min_gap=0.0, what='many, one file')
    st = dev.sites_cluster_last_stats()
    assert n == st['n_sites'] == st['n_mixed'] == bed.count(b'\n') > 1024 and st['n_link_small'] == n, st


def test_a_deep_key_that_is_not_kept_declines_nothing(dev, tmp_path):
    """8200 native rows against one control row at -d 2, and 9000 rows in the control alone: neither key is a site, so neither is
    over the cap, and neither is the deepest site.  With a second control row the first is a site and declines the file."""
    native, control, line = G.deep_pair(kept=False)
    _, _, n = device_makes_it(dev, tmp_path, native, control, depth=2, what='deep, not kept')
    st = dev.currents_compare_last_stats()
    assert n == 3 and (st['n_sites'], st['deepest_site'], st['n_columns']) == (3, 6, 1), st
    native, control, line = G.deep_pair(kept=True)
    host_does_it(dev, tmp_path, native, control, 'depth', 1, line, depth=2)
    assert 'native' in CC.last_compare['reason'] and 'line %d' % (line + 1) in CC.last_compare['reason']


def test_every_accepted_spelling_of_a_number(dev, tmp_path):
    native, control, native_twin, control_twin = G.spellings_pair()
    rows, _, n = device_makes_it(dev, tmp_path, native, control, depth=2, what='spellings')
    st = dev.currents_compare_last_stats()
    twin, _, n_twin = device_makes_it(dev, tmp_path, native_twin, control_twin, depth=2, what='repr twin')
    assert n == n_twin == 3 and rows == twin and st['n_columns'] == G.SPELLINGS_C
    blob, _, _, _, reason = dev.currents_compare(text1=native, text2=control_twin, depth=2)
    assert reason is None and blob == rows


def test_texts_without_a_site(dev, tmp_path):
    pairs = G.empty_pairs()
    for name in ('empty control', 'no shared key', 'all below depth', 'both empty'):
        native, control = pairs[name]
        assert dev.currents_compare(text1=native, text2=control, depth=3, by='t') == (b'', b'', 0, 0, None), name
        assert device_makes_it(dev, tmp_path, native, control, depth=3, by='t', what=name)[2] == 0
    # an empty native text has no first row to take the columns from: n_columns is 0, the control's first line has another number
    # of values, and the host statement writes the empty output
    native, control = pairs['empty native']
    host_does_it(dev, tmp_path, native, control, 'cur_values', 2, 0, depth=3)
    assert CC.last_compare == dict(by='host', reason=CC.last_compare['reason'], n_sites=0, n_sig=0)
    assert open(str(tmp_path / 'out.tsv'), 'rb').read() == b'' and dev.currents_compare_last_stats()['n_columns'] == 0
    # behind them the device serves as before
    native, control = pairs['no shared key'][0], pairs['empty native'][1]
    assert device_makes_it(dev, tmp_path, native, control, depth=3, what='behind the empty ones')[2] == 3


def test_a_column_declines_its_site(dev, tmp_path):
    """far_tail, tie and print of one column among ordinary ones; cu_tw_reason's order over a site's columns; the smallest head line
    among two declining sites; and a served call on the same Device behind them."""
    for name, (native, control, depth, reason, line) in G.combine_declines().items():
        host_does_it(dev, tmp_path, native, control, reason, 1, line, depth=depth)
        assert dev.currents_compare_last_stats()['decline_file'] == 1, name
    native, control = G.keys_pair()
    assert device_makes_it(dev, tmp_path, native, control, depth=3, what='behind the declines')[2] == 9
