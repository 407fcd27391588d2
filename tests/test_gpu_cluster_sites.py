"""cluster_sites on the GPU (mcaller_amd/csrc/compare/mc_sitecluster.inc, csrc/mc_linkage.h; Device.sites_cluster,
cluster_sites.cluster_sites_device) against the host statement: the device's bytes equal the host's, rows and bed, text to text and
file to file, with `reason is None` on every case that is not a decline; every decline with its reason and line and the host's output
or error behind it."""
import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import cluster_sites as CS
from tests import cluster_cases as K

pytestmark = pytest.mark.gpu

METRICS = ('correlation', 'euclidean')
WAVE, LDS, CAP = _lib.CLU_WAVE_ROWS, _lib.CLU_LDS_ROWS, _lib.CLU_MAX_DEPTH


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def device_makes_it(dev, tmp_path, text, depth=15, max_depth=256, metric='correlation', mixed=False, min_minor=0.2, min_gap=2.0, what=''):
    """The device's rows and bed equal the host statement's, from the text and from the file; -> (rows, bed, n_sites)."""
    p = K.write(tmp_path, text)
    want, want_bed, n, n_mixed = CS._rows(p, depth, max_depth, metric, mixed, min_minor, min_gap)
    blob, bed, n_sites, got_mixed, reason = dev.sites_cluster(text=text, depth=depth, max_depth=max_depth, metric=metric, mixed=mixed,
                                                              min_minor=min_minor, min_gap=min_gap)
    assert reason is None, (what, reason)
    assert blob == want and (n_sites, got_mixed) == (n, n_mixed) and bed == (want_bed or b''), what
    out, mixed_bed = str(tmp_path / 'out.tsv'), str(tmp_path / 'mixed.bed')
    assert CS.cluster_sites_device(p, out=out, depth=depth, max_depth=max_depth, metric=metric, mixed_bed=mixed_bed if mixed else None,
                                   min_minor=min_minor, min_gap=min_gap) == n
    assert CS.last_cluster == dict(by='device', reason=None, n_sites=n, n_mixed=n_mixed), (what, CS.last_cluster)
    assert open(out, 'rb').read() == want and (not mixed or open(mixed_bed, 'rb').read() == want_bed), what
    return want, want_bed, n


def host_does_it(dev, tmp_path, text, reason, line, error=None, **kw):
    """The device declines with the reason and line, and the host statement's output or error stands behind it."""
    p = K.write(tmp_path, text)
    out = str(tmp_path / 'out.tsv')
    if error is not None:
        with pytest.raises(ValueError, match=error):
            CS.cluster_sites_device(p, out=out, **kw)
    else:
        want, _, n, _ = CS._rows(p, kw.get('depth', 15), kw.get('max_depth', 256), kw.get('metric', 'correlation'))
        assert CS.cluster_sites_device(p, out=out, **kw) == n
        assert CS.last_cluster['by'] == 'host' and CS.last_cluster['reason'], CS.last_cluster
        assert open(out, 'rb').read() == want
    st = dev.sites_cluster_last_stats()
    assert (st['decline_reason'], st['decline_line']) == (_lib.CMP_DECLINE[reason], line), st


@pytest.mark.parametrize('metric', METRICS)
def test_link_kernel_edges(dev, tmp_path, metric):
    """Usable depths at the edges of the two wave instances (32, 64), of the LDS matrix and beyond it, three columns."""
    depths = [2, 3, 32, 33, 63, 64, 65, LDS, LDS + 1]
    text = K.depth_text(depths, c=3)
    _, _, n = device_makes_it(dev, tmp_path, text, depth=2, metric=metric, what='link edges')
    st = dev.sites_cluster_last_stats()
    assert n == len(depths) and (st['n_link_small'], st['n_link_lds'], st['n_link_slab'], st['deepest_site'], st['n_columns']) == (6, 2, 1, LDS + 1, 3), st
    assert st['slab_groups'] == 1 and st['slab_bytes'] == (LDS + 1) * ((LDS + 1) | 1) * 8


def test_the_depth_cap(dev, tmp_path):
    """max_depth rows and max_depth + 1 at the cap of 1024 (the slab kernel's largest site) and at a max_depth inside the LDS kernel."""
    text = K.depth_text([CAP, CAP + 1], c=3, seed=7)
    rows, _, n = device_makes_it(dev, tmp_path, text, depth=2, max_depth=CAP, what='cap')
    f = [r.split('\t') for r in rows.decode().splitlines()]
    assert n == 2 and [r[5] for r in f] == [str(CAP), str(CAP + 1)] and all(int(r[7]) + int(r[8]) == CAP for r in f)
    st = dev.sites_cluster_last_stats()
    assert (st['n_link_slab'], st['deepest_site'], st['slab_groups']) == (2, CAP, 2), st
    text = K.depth_text([100, 101, 99], c=3, seed=9)
    rows, _, n = device_makes_it(dev, tmp_path, text, depth=100, max_depth=100, metric='euclidean', what='max_depth 100')
    assert n == 2 and [r.split('\t')[5] for r in rows.decode().splitlines()] == ['100', '101']
    assert dev.sites_cluster_last_stats()['n_link_lds'] == 2


@pytest.mark.parametrize('metric', METRICS)
def test_interleaved_sites(dev, tmp_path, metric):
    """About 2000 lines of 80 sites shuffled together: every site's rows lie in several 256-line tiles and arrive in no order."""
    text = K.seeded_text(80, 5, 45, seed=13)
    assert text.count(b'\n') > 1500
    _, bed, n = device_makes_it(dev, tmp_path, text, depth=8, metric=metric, mixed=True, min_gap=1.3, what='interleaved')
    assert 60 <= n <= 80 and 0 < bed.count(b'\n') < n


@pytest.mark.parametrize('metric', METRICS)
def test_equal_distances_everywhere(dev, tmp_path, metric):
    """Duplicated rows (distance 0.0), all-identical rows in every link kernel (the index rule decides every merge), small-integer
    vectors whose distances tie all the time -- in the wave kernels, the LDS kernel and the slab kernel."""
    rng = np.random.default_rng(19)
    X = K.gaussian(rng, 9)
    groups = [K.site_lines('c', 5, '+', np.vstack([X, X[2], X[2], X[5], X]))]
    groups += [K.site_lines('c', 10 + n, '-', np.tile(K.gaussian(rng, 1), (n, 1))) for n in (9, 40, 70, LDS + 4)]
    groups += [K.site_lines('d', 10 + n, '+', K.integers(rng, n, K.C6, 1)) for n in (5, 12, 30, 50, 64, 90, 160)]
    _, _, n = device_makes_it(dev, tmp_path, K.text_of(groups, rng), depth=4, metric=metric, what='ties')
    assert n == len(groups)
    st = dev.sites_cluster_last_stats()
    assert st['n_link_lds'] >= 2 and st['n_link_slab'] >= 1


def test_flat_rows_move_the_anchor(dev, tmp_path):
    """Three constant rows in front of every site: flat under correlation, so cluster 1's anchor is the fourth row and the usable
    depths are those of test_link_kernel_edges; under euclidean they are rows."""
    depths = [2, 29, 61, 62, LDS - 3, LDS - 2]
    text = K.depth_text(depths, c=4, metric_flat=3)
    rows, _, n = device_makes_it(dev, tmp_path, text, depth=2, what='flat')
    assert n == len(depths) and all(r.split('\t')[6] == '3' for r in rows.decode().splitlines())
    assert dev.sites_cluster_last_stats()['n_link_small'] == 4
    rows, _, n = device_makes_it(dev, tmp_path, text, depth=5, metric='euclidean', what='flat, euclidean')
    assert n == len(depths) and dev.sites_cluster_last_stats()['n_link_small'] == 3
    only_flat = K.text_of([K.site_lines('c', 5, '+', np.full((6, 4), 2.0))])
    assert device_makes_it(dev, tmp_path, only_flat, depth=2, what='flat alone')[2] == 0


@pytest.mark.parametrize('c', [2, 7])
def test_two_and_seven_columns(dev, tmp_path, c):
    text = K.seeded_text(30, 4, 70, seed=23, c=c)
    for metric in METRICS:
        assert device_makes_it(dev, tmp_path, text, depth=4, metric=metric, what='c = %d' % c)[2] == 30


def test_mixed_bed_at_its_thresholds(dev, tmp_path):
    """Thresholds taken from the rows themselves: a site sits exactly on each, others lie on both sides; a site of two usable rows
    has h_sub == 0.0 and passes any gap."""
    rng = np.random.default_rng(31)
    text = K.seeded_text(40, 6, 30, seed=29, planted=2) + K.text_of([K.site_lines('e', 5, '+', K.gaussian(rng, 2))])
    rows = [r.split('\t') for r in CS._rows(K.write(tmp_path, text), 2)[0].decode().splitlines()]
    assert rows[-1][0] == 'e' and rows[-1][12] == '0.0'
    minor = sorted(min(int(r[7]), int(r[8])) / (int(r[7]) + int(r[8])) for r in rows)
    gap = sorted(float(r[11]) / float(r[12]) for r in rows if float(r[12]) > 0.0)
    for min_minor, min_gap in [(minor[len(minor) // 2], 1.0), (0.0, gap[len(gap) // 2]), (minor[len(minor) // 3], gap[len(gap) // 3]), (0.5, 0.0)]:
        _, bed, n = device_makes_it(dev, tmp_path, text, depth=2, mixed=True, min_minor=min_minor, min_gap=min_gap, what=(min_minor, min_gap))
        assert n == 41 and 0 < bed.count(b'\n') < n
        assert b'\ne\t5\t' in b'\n' + bed


def test_hash_collisions(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', 'f')
    text = K.seeded_text(40, 3, 8, seed=37, c=3)
    assert device_makes_it(dev, tmp_path, text, depth=3, what='sixteen chains')[2] >= 30
    assert dev.sites_cluster_last_stats()['longest_probe'] > 2


@pytest.mark.parametrize('ending', ['newline', 'none'])
def test_small_stages_and_the_last_line(dev, tmp_path, monkeypatch, ending):
    monkeypatch.setenv('MCALLER_TEXT_STAGE_BYTES', '1000')
    text = K.seeded_text(25, 4, 12, seed=41)
    if ending == 'none':
        text = text[:-1]
    assert len(text) > 10000
    assert device_makes_it(dev, tmp_path, text, depth=4, what=ending)[2] >= 20


def test_declines_with_reason_and_line(dev, tmp_path):
    text = K.seeded_text(6, 4, 6, seed=43, shuffle=False).decode()
    n = text.count('\n')
    good = K.row('chr9', 5, '+', [0.5, 0.25, 1.0, -1.0, 2.0, 0.0], prob=0.25)
    cases = [('cur_fields', text + 'chr9\tr\t5\n', n, '3 tab-separated fields'),
             ('cur_values', text + good.replace('0.5,', ''), n, '6 values, 7 are expected'),
             ('cur_pos', text + good.replace('\t5\t', '\t+5\t'), n, None),                       # int() takes it: the host does the file
             ('cur_pos', text + good.replace('\t5\t', '\t5x\t'), n, 'a position that is no integer'),
             ('number', text + good.replace('0.25,', '0.2_5,'), n, None),
             ('number', text + good.replace('0.25,', 'inf,'), n, 'a value that is not finite'),
             ('number', text + good.replace('9.5', 'nan'), n, 'a value that is not finite'),     # the read quality is parsed too
             ('number', text + good.replace('0.25,', '1e999,'), n, 'a value that is not finite'),
             ('high_byte', text + good.replace('GATCM', 'GATéM'), n, None),
             ('control', good.replace('GATCM', 'GA\x01CM') + text, 0, None),
             ('long_line', text + good.replace('read1', 'r' * 70000), n, None),
             ('cur_values', K.row('chr9', 5, '+', [0.5]) * 3, 0, 'at least 3 are needed')]
    for reason, bad, line, error in cases:
        host_does_it(dev, tmp_path, bad.encode('utf-8'), reason, line, error, depth=4)
    # a height the row writer does not print: two rows 2e9 apart under euclidean
    far = K.text_of([K.site_lines('c', 5, '+', [[0.0, 0.0, 0.0], [2e9, 0.0, 1.0], [1.0, 2.0, 3.0]])])
    host_does_it(dev, tmp_path, far, 'print', 0, depth=2, metric='euclidean')
    assert device_makes_it(dev, tmp_path, far, depth=2, what='the same rows under correlation')[2] == 1


def shared_stage_pair():
    """Two files of 3 sites each with 3 .. 5 rows a site, the sites' rows interleaved: two shared sites, one in the native file alone (a
    key with no control count), one in the control alone (a key no native line is the first of); the native file lacks its last newline."""
    from tests import currents_cases as KC
    native, control = KC.seeded_pair(2, 3, 5, seed=67, c=3)
    return native[:-1], control


def test_currents_and_cluster_take_turns_on_one_device(dev, tmp_path, monkeypatch):
    """compare_currents and cluster_sites share the site-grouping stage (mc_sitegroup.inc): on one Device a comparison, a clustering of
    its native file, and both again give the host statements' bytes each time -- nothing of one call's grouping is left for the next.
    The keys share probe chains (four slots of hash); a key table too small declines both, and the calls behind it are as before."""
    from mcaller_amd import compare_currents as CC
    from tests import currents_cases as KC
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', '3')
    native, control = shared_stage_pair()
    p1, p2 = KC.files(tmp_path, native, control)
    rows, bed, n, n_sig = CC._rows(p1, p2, 3, False, 't', 0.0, True)
    c_rows, c_bed, c_n, c_mixed = CS._rows(p1, 3, 256, 'correlation', True, 0.0, 0.0)
    assert n == 2 and c_n == 3 and not native.endswith(b'\n')

    def compare():
        return dev.currents_compare(text1=native, text2=control, depth=3, by='t', threshold=0.0)

    def cluster():
        return dev.sites_cluster(text=native, depth=3, mixed=True, min_minor=0.0, min_gap=0.0)

    first, second, third, fourth = compare(), cluster(), compare(), cluster()
    assert first == (rows, bed or b'', n, n_sig, None), first
    assert second == (c_rows, c_bed or b'', c_n, c_mixed, None), second
    assert third == first and fourth == second
    assert dev.currents_compare_last_stats()['longest_probe'] > 1 and dev.sites_cluster_last_stats()['longest_probe'] > 1
    monkeypatch.setenv('MCALLER_CMP_TABLE_SLOTS', '2')                 # four keys, three in the native file
    assert compare()[0] is None and cluster()[0] is None
    assert dev.currents_compare_last_stats()['decline_reason'] == _lib.CMP_DECLINE['table']
    assert dev.sites_cluster_last_stats()['decline_reason'] == _lib.CMP_DECLINE['table']
    monkeypatch.delenv('MCALLER_CMP_TABLE_SLOTS')
    assert compare() == first and cluster() == second


def test_table_memory_and_slab_declines_then_two_calls_and_release(dev, tmp_path, monkeypatch):
    text = K.seeded_text(40, 3, 4, seed=53, c=2)
    p = K.write(tmp_path, text)
    monkeypatch.setenv('MCALLER_CMP_TABLE_SLOTS', '16')
    assert dev.sites_cluster(path=p, depth=3)[0] is None
    assert dev.sites_cluster_last_stats()['decline_reason'] == _lib.CMP_DECLINE['table']
    monkeypatch.delenv('MCALLER_CMP_TABLE_SLOTS')
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', '4096')
    assert dev.sites_cluster(path=p, depth=3)[0] is None
    assert dev.sites_cluster_last_stats()['decline_reason'] == _lib.CMP_DECLINE['memory']
    # room for everything but the slab of a site of 600 rows (2.9 MB); with 5 MB there is one slab (2.9 MB and the
    # megabyte every request is counted with) for the two deep sites, not two
    deep = K.depth_text([600, 20, 500], c=2, seed=3)
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', str(2 << 20))
    host_does_it(dev, tmp_path, deep, 'memory', -1, depth=2, max_depth=1024)
    assert 'slab' in CS.last_cluster['reason']
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', str(5 << 20))
    assert device_makes_it(dev, tmp_path, deep, depth=2, max_depth=1024, what='one slab')[2] == 3
    st = dev.sites_cluster_last_stats()
    assert (st['n_link_slab'], st['slab_groups']) == (2, 1), st
    monkeypatch.delenv('MCALLER_CMP_DEVICE_BYTES')
    assert device_makes_it(dev, tmp_path, text, depth=3)[2] >= 30
    assert device_makes_it(dev, tmp_path, text, depth=3, metric='euclidean')[2] >= 30
    dev.sites_cluster_release()
    assert device_makes_it(dev, tmp_path, text, depth=3)[2] >= 30
    assert device_makes_it(dev, tmp_path, b'', depth=3, what='an empty file')[2] == 0
