"""compare_genomes --fisher --fdr on the GPU (mcaller_amd/csrc/compare/mc_cmpfdr.inc; Device.fisher_exact, Device.bh_adjust,
compare_genomes.compare_by_position_device) against the host statement: the device's bytes equal the host's, text to text and file
to file, at the sort's and the scans' block and round edges, on planted tables and at the depth edges; every decline with its
reason and the host's bytes or error behind it; mc_fisher_exact_device against the host build, mc_bh_adjust_device against
bh_log10."""
import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import compare_genomes as CG
from tests import fisher_bh_cases as F
from tests import gpu_compare_cases as GC

pytestmark = pytest.mark.gpu

FAR_TAIL = _lib.ABI.constants['MC_FISHER_FAR_TAIL']
BH_TIE, BH_RANGE = _lib.ABI.constants['MC_BH_TIE'], _lib.ABI.constants['MC_BH_RANGE']
BH_SLACK = 1.0e-13                            # mc_bh.h's derived slack of the terms
FLAGS = [dict(fisher=True), dict(fdr=True), dict(fisher=True, fdr=True)]


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def files(tmp_path, t1, t2):
    p1, p2 = str(tmp_path / 'a.bed'), str(tmp_path / 'b.bed')
    open(p1, 'wb').write(t1)
    open(p2, 'wb').write(t2)
    return p1, p2


def host_rows(p1, p2, lift):
    """The host statement's bytes for each of FLAGS from one run with both (tests/test_fisher_bh.py holds the columns of every
    combination to be these), and the number of rows."""
    both, n = CG.compare_rows(p1, p2, fisher=True, fdr=True, **lift)
    rows = [line.split('\t') for line in both.decode().splitlines()]
    k = len(rows[0]) - 6 if rows else 0                           # the columns up to nlp_ks
    pick = lambda cols: ''.join('\t'.join(cols(r)) + '\n' for r in rows).encode()
    return {(True, False): pick(lambda r: r[:k + 1]), (False, True): pick(lambda r: r[:k] + r[k + 1:k + 5]), (True, True): both}, n


def device_makes_it(tmp_path, t1, t2, flag_sets, what='', lift=None):
    """For every set of flags the device's file equals the host statement's, and last_compare names the device."""
    p1, p2 = (t1, t2) if lift else files(tmp_path, t1, t2)
    lift = lift or {}
    flag_sets = [flag_sets] if isinstance(flag_sets, dict) else flag_sets
    wants, n = host_rows(p1, p2, lift)
    out = str(tmp_path / 'out.tsv')
    for flags in flag_sets:
        fisher, fdr = bool(flags.get('fisher')), bool(flags.get('fdr'))
        assert CG.compare_by_position_device(p1, p2, out=out, **lift, **flags) == n, what
        assert (CG.last_compare['by'], CG.last_compare['reason']) == ('device', None), (what, flags, CG.last_compare)
        assert (CG.last_compare['fisher'], CG.last_compare['fdr']) == (fisher, fdr)
        assert open(out, 'rb').read() == wants[fisher, fdr], (what, flags)
    return n


def host_does_it(tmp_path, t1, t2, flags, reason):
    """The device declines with `reason` in its words and the host statement's bytes are written."""
    p1, p2 = files(tmp_path, t1, t2)
    want, n = CG.compare_rows(p1, p2, **flags)
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(p1, p2, out=out, **flags) == n
    assert CG.last_compare['by'] == 'host' and reason in CG.last_compare['reason'], CG.last_compare
    assert open(out, 'rb').read() == want


@pytest.mark.parametrize('n_sites', [1, 2, 255, 256, 257, 1023, 1024, 1025, 1100])
def test_site_counts_at_the_block_and_round_edges(dev, tmp_path, n_sites):
    t1, t2 = F.counted_pair(F.planted_tables(n_sites))
    assert device_makes_it(tmp_path, t1, t2, FLAGS, 'sites %d' % n_sites) == n_sites


@pytest.mark.parametrize('order', ['ascending', 'descending'])
def test_bed1_in_order_of_p(dev, tmp_path, order):
    tables = F.planted_tables(300)
    L = _lib.fisher_exact(*np.asarray(tables, dtype=np.int64).T)[0]
    at = np.argsort(L, kind='stable')
    t1, t2 = F.counted_pair([tables[i] for i in (at if order == 'ascending' else at[::-1])])
    device_makes_it(tmp_path, t1, t2, FLAGS, order)


def test_equal_columns_and_ties_across_a_block(dev, tmp_path):
    """Every site the same two lines' values and counts: all five columns are all-equal columns.  Then 600 sites of three kinds
    in turn: tie groups of 200 that straddle the blocks of 256."""
    one = F.planted_tables(7)[6]
    t1, t2 = F.counted_pair([one] * 300)
    same1 = t1.decode().splitlines()[0].split('\t')
    same2 = t2.decode().splitlines()[0].split('\t')
    def lines(fields, k):
        return ''.join('\t'.join([fields[0], str(1000 + 7 * i), str(1001 + 7 * i)] + fields[3:]) + '\n' for i in range(k)).encode()
    device_makes_it(tmp_path, lines(same1, 300), lines(same2, 300), FLAGS, 'all equal')
    kinds = F.planted_tables(9)[6:9]
    a, b = F.counted_pair(kinds)
    a, b = [l.split('\t') for l in a.decode().splitlines()], [l.split('\t') for l in b.decode().splitlines()]
    def mixed(rows):
        return ''.join('\t'.join([rows[i % 3][0], str(1000 + 7 * i), str(1001 + 7 * i)] + rows[i % 3][3:]) + '\n' for i in range(600)).encode()
    device_makes_it(tmp_path, mixed(a), mixed(b), dict(fisher=True, fdr=True), 'tie groups')


def test_depth_edges_with_planted_counts(dev, tmp_path):
    """The sites of GC.EDGE_SIZES (pooled 3 .. 8192) with counts planted through frac, independent of the probabilities."""
    rng = np.random.default_rng(67)
    sites = [GC.T.sample('round2', n1, n2, GC.EDGE_SEED) for n1, n2 in GC.EDGE_SIZES]
    l1, l2 = [], []
    for i, (x, y) in enumerate(sites):
        f = rng.random()
        K1, K2 = int(rng.binomial(len(x), f)), int(rng.binomial(len(y), min(1.0, f + 0.03)))
        l1.append(F.counted_line('chr1', 1000 + 7 * i, '+', K1, len(x), values=x))
        l2.append(F.counted_line('chr1', 1000 + 7 * i, '+', K2, len(y), values=y))
    device_makes_it(tmp_path, ''.join(l1).encode(), ''.join(l2).encode(), FLAGS, 'depth edges')


def test_through_an_alignment(dev, tmp_path):
    P, lift, n = F.lifted_files(tmp_path)
    assert device_makes_it(tmp_path, P['bed1'], P['bed2'], FLAGS, 'xmfa', lift=lift) == n
    assert 'n_unaligned' in CG.last_compare


@pytest.mark.parametrize('which', [1, 2])
def test_a_frac_that_is_no_count_declines_on_a_shared_line_only(dev, tmp_path, which):
    ok1, ok2 = F.counted_pair(F.planted_tables(5))
    bad, good = F.counted_line('chr1', 50000, '+', 0, 9, frac='0.3333').encode(), F.counted_line('chr1', 50000, '+', 3, 9, values=np.round(np.random.default_rng(71).random(9), 2)).encode()
    t1, t2 = (ok1 + bad, ok2 + good) if which == 1 else (ok1 + good, ok2 + bad)
    p1, p2 = files(tmp_path, t1, t2)
    with pytest.raises(ValueError, match='^bed%d line 6: frac is not a count over its reads$' % which):
        CG.compare_by_position_device(p1, p2, out=str(tmp_path / 'out.tsv'), fisher=True)
    st = dev.bed_compare_last_stats()
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['frac'], which, 5)
    want, n = CG.compare_rows(p1, p2, fdr=True)                             # frac is not read without --fisher
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(p1, p2, out=out, fdr=True) == n == 6
    assert CG.last_compare['by'] == 'device' and open(out, 'rb').read() == want
    alone = F.counted_line('chr1', 60000, '+', 0, 9, frac='0.3333').encode()
    t1, t2 = (ok1 + alone, ok2) if which == 1 else (ok1, ok2 + alone)
    assert device_makes_it(tmp_path, t1, t2, dict(fisher=True), 'an unshared line') == 5


def test_far_tail_declines(dev, tmp_path):
    x, y = GC.T.sample('round2', 4000, 4192, 5)
    ok1, ok2 = F.counted_pair(F.planted_tables(3))
    t1 = ok1 + F.counted_line('chr1', 70000, '+', 4000, 4000, values=x).encode()
    t2 = ok2 + F.counted_line('chr1', 70000, '+', 0, 4192, values=y).encode()
    host_does_it(tmp_path, t1, t2, dict(fisher=True, fdr=True), "Fisher's test: -250")
    st = dev.bed_compare_last_stats()
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['far_tail'], 1, 3)


def test_without_the_flags_nothing_changes(dev, tmp_path):
    t1, t2 = GC.edge_pair()
    p1, p2 = files(tmp_path, t1, t2)
    want, n = CG.compare_rows(p1, p2)
    blob, n_sites, reason = dev.bed_compare(text1=t1, text2=t2)
    assert reason is None and blob == want and n_sites == n
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(p1, p2, out=out) == n
    assert CG.last_compare == dict(by='device', reason=None, n_sites=n) and open(out, 'rb').read() == want


def test_device_build_of_fishers_test_against_the_host_build(dev):
    """The CPU test's grid: every value within the sum of the two bounds, every status the host build's."""
    tables = F.small_tables() + [c[1:] for c in F.seeded_tables()]
    K1, n1, K2, n2 = np.asarray(tables, dtype=np.int64).T
    hl, hb, hs = _lib.fisher_exact(K1, n1, K2, n2)
    dl, db, ds = dev.fisher_exact(K1, n1, K2, n2)
    assert np.array_equal(hs, ds)
    ok = np.isfinite(hb)
    assert np.all(np.abs(hl[ok] - dl[ok]) <= hb[ok] + db[ok])
    assert np.array_equal(hl[~ok], dl[~ok]) and np.array_equal(hb[~ok], db[~ok])
    print('bits equal: %s; largest |device - host|: %.3g' % (bool(np.array_equal(hl, dl) and np.array_equal(hb, db)), np.max(np.abs(hl[ok] - dl[ok]))))
    assert int(ds[-3]) == FAR_TAIL and dl[-3] == -np.inf
    bad = dev.fisher_exact([6], [5], [1], [3])
    assert bad[2][0] == _lib.ABI.constants['MC_FISHER_BAD_ARGS'] and np.isnan(bad[0][0])


@pytest.mark.parametrize('n', [1, 2, 256, 257, 2048, 2049, 65537])
def test_device_build_of_the_adjustment(dev, n):
    L = F.device_column(n)
    bound = np.full(n, 1e-15)
    Q, rounded, st = dev.bh_adjust(L, bound)
    with np.errstate(all='ignore'):
        want = CG.bh_log10(L)
    assert np.array_equal(np.isnan(Q), np.isnan(want)) and np.array_equal(np.isnan(rounded), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(Q[ok] - want[ok]) <= BH_SLACK), np.max(np.abs(Q[ok] - want[ok]))
    assert np.array_equal(rounded[ok], np.round(0.0 - Q[ok], 3))
    for v in np.unique(L[ok])[:50]:
        assert len(set(Q[L == v])) == 1                                    # planted ties: one Q
    hQ, hr, hst = _lib.bh_adjust(L, bound)
    assert np.all(np.abs(Q[ok] - hQ[ok]) <= 2 * BH_SLACK)
    if not (st & BH_TIE):
        assert [str(v) for v in rounded] == [str(np.round(0.0 - q, 3)) for q in want]


def test_adjustment_statuses_on_the_device(dev):
    Q, rounded, st = dev.bh_adjust([-1.2345], [1e-9])
    assert st == BH_TIE and Q[0] == -1.2345 and rounded[0] in (1.234, 1.235)
    assert dev.bh_adjust([-1.2341], [1e-9])[2] == 0
    assert dev.bh_adjust([-1.2345, -3.0], [0.0, 1e-9])[2] == BH_TIE
    for L, b in [([0.5, -1.0], [0.0, 0.0]), ([-400.0], [0.0]), ([-1.0], [-1.0]), ([-1.0], [np.inf])]:
        Q, rounded, st = dev.bh_adjust(L, b)
        assert st == BH_RANGE and np.isnan(Q).all() and np.isnan(rounded).all()
    Q, rounded, st = dev.bh_adjust(np.full(300, np.nan), np.zeros(300))
    assert st == 0 and np.isnan(Q).all()
    Q, rounded, st = dev.bh_adjust(np.full(700, -2.5), np.zeros(700))         # an all-equal column: no pass of the sort runs
    assert st == 0 and np.all(Q == -2.5) and np.all(rounded == 2.5)


def test_too_little_memory_for_the_sort_buffers(dev, monkeypatch):
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', str(1 << 16))
    with pytest.raises(_lib.McError, match='do not fit'):
        dev.bh_adjust(np.full(5000, -1.0), np.zeros(5000))


def test_the_pipeline_counts_its_sort_buffers(dev, tmp_path, monkeypatch):
    """The least MCALLER_CMP_DEVICE_BYTES at which the files compare without the flags (found by bisection; shallow sites, so the
    per-site tables are what it is set by) is too little with them: the columns and the sort buffers are counted on top."""
    t1, t2 = F.counted_pair(F.planted_tables(1100, top=3))
    def fits(budget, **flags):
        monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', str(budget))
        return dev.bed_compare(text1=t1, text2=t2, **flags)[0] is not None
    lo, hi = 1 << 16, 1 << 26
    assert not fits(lo) and fits(hi) and fits(hi, fisher=True, fdr=True)
    while hi - lo > 4096:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fits(mid) else (mid, hi)
    assert fits(hi) and not fits(hi, fisher=True, fdr=True)
    st = dev.bed_compare_last_stats()
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['memory'], 0, -1)
    p1, p2 = files(tmp_path, t1, t2)
    want, n = CG.compare_rows(p1, p2, fisher=True, fdr=True)
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(p1, p2, out=out, fisher=True, fdr=True) == n == 1100
    assert CG.last_compare['by'] == 'host' and 'memory' in CG.last_compare['reason'] and open(out, 'rb').read() == want


def test_the_command_line(dev, tmp_path):
    t1, t2 = F.counted_pair(F.planted_tables(40))
    p1, p2 = files(tmp_path, t1, t2)
    out = str(tmp_path / 'out.tsv')
    CG.main(['--bed1', p1, '--bed2', p2, '-o', out, '--fisher', '--fdr', '--device'])
    assert open(out, 'rb').read() == CG.compare_rows(p1, p2, fisher=True, fdr=True)[0]
    assert CG.last_compare == dict(by='device', reason=None, n_sites=40, fisher=True, fdr=True)
