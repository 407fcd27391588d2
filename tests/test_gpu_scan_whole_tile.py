"""k1_scan's whole-tile path: the instances that stream unit summaries (a table's first pass under a sparse motif, mode 3, and
every later pass, mode 2) take a tile that lies inside ONE name block in a single batch.  The tables of tests/whole_tile_cases.py
(three tiles plus 1, 3 or 7 rows) on the synchronous pass, the pipelined first pass, the pass behind it, the first pass declared new
and the pass behind that, under GATC and GTAC; every record is the C oracle's, every pass is asked which instance it took, and
after the synchronous pass the library says which tiles satisfy the path's predicate (mc_ctx_whole_tiles) -- a tile that is not
on the path its case was written for fails the case.
(a) the edges of the predicate; (b) a window's last row on the former chunk edge, the stripe edges and the tile's last rows,
closed by the next row or behind one or two filtered rows; (c) one violating pair inside a path tile: the pass is repeated;
(d) a tile that lists more than 64 units but no more than 64 per chunk: the general loop takes it; (e) a slot that held a longer
table whose path tile now holds a block edge.  Runs on a real MI355X only."""
import numpy as np
import pytest

from tests import edge_tables as E
from tests import helpers as H
from tests import whole_tile_cases as W

pytestmark = pytest.mark.gpu
FIRST_MODE, LATER_MODE = 3, 2


@pytest.fixture()
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope='module')
def weights():
    from mcaller_amd import extract_contexts as ec
    _, w, _, soc = ec.submodel_setup(H.load_modelset('r95'), 'A')
    return w, soc


def scored_oracle(case, arrays, weights):
    orc = H.oracle_records(case.table, arrays, case.qual, W.K, W.SKIP, case.qual_thresh)
    H.oracle_score(orc, case.table, case.qual, weights[0], weights[1], W.K)
    return orc


def synchronous(dev, table, qual, qual_thresh, whole, what):
    """The synchronous pass, and which tiles its descriptors put on the path."""
    dev.upload_table(table)
    dev.set_read_quality(qual)
    rec = dev.extract(W.K, W.SKIP, qual_thresh)
    got = dev.whole_tiles(table.n_rows).tolist()
    assert got == whole, '%s: tiles on the path %r, the case was written for %r' % (what, got, whole)
    return rec


def passes(dev, case, orc, what=None):
    what = what or case.name

    def compare(rec, how):
        try:
            H.assert_records_equal(rec, orc, W.K, prob_tol=1e-6)
        except AssertionError as e:
            raise AssertionError('%s, %s: %s' % (what, how, e))
    if 'unbroken' in case.more:             # (the violating table's blocks end up irregular: its twin says the tile was a regular block's)
        synchronous(dev, case.more['unbroken'], case.qual, case.qual_thresh, case.whole, what + ', unbroken')
    compare(synchronous(dev, case.table, case.qual, case.qual_thresh, case.whole, what), 'synchronous first pass')
    slot = dev.upload_table_async(case.table, case.qual)
    for as_new in (False, True):
        if as_new:
            dev.select_table(slot, as_new=True)
        how = 'first pass%s' % (' (declared new)' if as_new else '')
        dev.run_async(W.K, W.SKIP, case.qual_thresh)
        assert dev.last_scan_mode() == FIRST_MODE, '%s, %s: scan mode %d' % (what, how, dev.last_scan_mode())
        rec = dev.wait()
        assert dev.last_pass_info()[1] == case.repeated, '%s, %s: the pass was %srepeated' % (what, how, 'not ' if case.repeated else '')
        compare(rec, how)
        dev.run_async(W.K, W.SKIP, case.qual_thresh)
        assert dev.last_scan_mode() == LATER_MODE, '%s, the pass behind the %s: scan mode %d' % (what, how, dev.last_scan_mode())
        compare(dev.wait(), 'the pass behind the ' + how)
    dev.sync()
    return slot


def run_cases(dev, motif, cases, weights):
    ref = E.ref_of(motif)
    dev.set_reference(ref.arrays)
    dev.set_mlp(*weights)
    n_rec = 0
    for c in cases:
        orc = scored_oracle(c, ref.arrays, weights)
        assert orc.n > 0, c
        n_rec += orc.n
        passes(dev, c, orc)
    assert n_rec > len(cases)


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_the_edges_of_the_predicate(dev, motif, weights):
    run_cases(dev, motif, W.eligibility_cases(motif, W.size_of(motif, 0)), weights)


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_a_windows_last_row_on_the_former_chunk_edge(dev, motif, weights):
    cases = W.chunk_edge_cases(motif, W.size_of(motif, 1))
    run_cases(dev, motif, cases, weights)


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_a_violating_pair_inside_a_path_tile(dev, motif, weights):
    run_cases(dev, motif, W.violation_cases(motif, W.size_of(motif, 2)), weights)


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_a_tile_that_lists_more_units_than_the_list_holds(dev, motif, weights):
    """The predicate holds, the tile lists 65 .. 128 units, at most 64 in either chunk: the general chunk loop takes it."""
    c = W.rich_case(motif, W.size_of(motif, 3))
    a, b = c.more['units']
    assert W.CG < a + b <= 2 * W.CG and a <= W.CG and b <= W.CG
    dev.set_reference(c.more['arrays'])
    dev.set_mlp(*weights)
    orc = scored_oracle(c, c.more['arrays'], weights)
    assert orc.n > 40
    passes(dev, c, orc)


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_a_slot_that_held_a_table_with_a_path_tile(dev, motif, weights):
    ref = E.ref_of(motif)
    dev.set_reference(ref.arrays)
    dev.set_mlp(*weights)
    longer, shorter = W.slot_reuse_tables(motif)
    orc_l, orc_s = scored_oracle(longer, ref.arrays, weights), scored_oracle(shorter, ref.arrays, weights)
    slot0 = passes(dev, longer, orc_l)
    synchronous(dev, shorter.table, shorter.qual, 0.0, shorter.whole, shorter.name)
    for _ in range(16):                                 # (the slots are taken in turn)
        slot = dev.upload_table_async(shorter.table, shorter.qual)
        if slot == slot0:
            break
        dev.sync()
    assert slot == slot0, 'the shorter table never went to slot %d' % slot0
    for mode in (FIRST_MODE, LATER_MODE):
        dev.run_async(W.K, W.SKIP, 0.0)
        assert dev.last_scan_mode() == mode
        H.assert_records_equal(dev.wait(), orc_s, W.K, prob_tol=1e-6)
    dev.sync()
