"""Reads, windows and violations placed on every edge at which the kernels cut a table (tests/edge_tables.py: units of 8 rows,
stripes and rounds of 512, pieces of 960, chunks of 1024, tiles of 2048), through the C ABI against the C oracle -- integers and
slot means bit for bit -- in every way a table is scanned: synchronous first pass, pipelined second and third pass, and, declared
new, two validating passes in flight; under a sparse motif (k1_scan<64> + k1_emit) and a one-base motif (k1_scan<130> +
k1_emit_runs; pipelined: k1_fused, and the library is asked that it ran so and was not repeated).  That the events lie where they
are said to lie is tests/test_edge_tables.py's business (CPU).  A failure names the table, the pass and the claims nearest to the
first record that differs.  Runs on a real MI355X only."""
import numpy as np
import pytest

from tests import edge_tables as E
from tests import helpers as H

pytestmark = pytest.mark.gpu
MOTIFS = ('GATC', 'A')


@pytest.fixture()
def dev():
    """(a context of its own per test: what an earlier pass ran out of decides which kernels the next one runs)"""
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope='module')
def weights():
    from mcaller_amd import extract_contexts as ec
    _, w, _, soc = ec.submodel_setup(H.load_modelset('r95'), 'A')
    return w, soc


def first_difference(got, want, k):
    """close_row of the first record of the oracle that the device's records do not show as it is (None: the counts differ only)."""
    if getattr(got, 'call_row', None) is not None:
        got = got.by_record()
    n = min(got.n, want.n)
    bad = np.zeros(n, dtype=bool)
    for name in ('site_pos', 'site_seg', 'close_row', 'info'):
        bad |= getattr(got, name)[:n] != getattr(want, name)[:n]
    bad |= (got.feats[:n * k].view(np.uint64) != want.feats[:n * k].view(np.uint64)).reshape(n, k).any(axis=1)
    bad |= ~((got.prob[:n] == want.prob[:n]) | (np.isnan(got.prob[:n]) & np.isnan(want.prob[:n])) | (np.abs(got.prob[:n] - want.prob[:n]) <= 1e-6))
    if bad.any():
        return int(want.close_row[int(np.flatnonzero(bad)[0])])
    return int(want.close_row[n]) if want.n > n else None


def compare(rec, orc, et, how, score):
    if not score:
        rec.prob[:rec.n] = np.nan
        orc.prob[:orc.n] = np.nan
    try:
        H.assert_records_equal(rec, orc, et.k, prob_tol=1e-6)
    except AssertionError as e:
        at = first_difference(rec, orc, et.k)
        raise AssertionError('%s: %s\n  %s' % (how, e, et.describe(at if at is not None else et.table.n_rows)))


def oracle(et, tail, score, weights):
    orc = H.oracle_records(et.table, et.ref.arrays, et.qual, et.k, et.skip, 0.0, tail_contig=tail)
    if score:
        H.oracle_score(orc, et.table, et.qual, weights[0], weights[1], et.k)
    return orc


def how_it_ran(dev, et, how):
    """A pipelined pass over a one-base motif ran as k1_fused and was not repeated -- unless a claim of the table says it must be
    (a slot of more than 128 events); a sparse motif: repeated exactly when the table says so."""
    room, rerun = dev.last_pass_info()
    if len(et.motif) == 1 and not et.rerun:
        assert room > 0, '%s, %s: the pass did not run as the fused kernel (room %d)' % (et.name, how, room)
    assert rerun == et.rerun, '%s, %s: repeated %r, expected %r' % (et.name, how, rerun, et.rerun)


def every_way(dev, et, weights, score=False, tails=None):
    """The sequence of test_one_base_motif_with_short_reads: synchronous first pass (validating), pipelined second, third (unit
    summaries under a sparse motif), and, declared new, two validating passes in flight."""
    dev.upload_table(et.table)
    dev.set_read_quality(et.qual)
    slot = dev.current_slot()
    for tail in tails or (et.tail,):
        orc = oracle(et, tail, score, weights)
        if tail != (tails or (et.tail,))[0]:
            dev.select_table(slot, as_new=True)
        compare(dev.extract(et.k, et.skip, 0.0, tail_contig=tail, score=score), orc, et, 'synchronous first pass, tail_contig %d' % tail, score)
        for again in range(4):
            if again == 2:
                dev.select_table(slot, as_new=True)
            dev.run_async(et.k, et.skip, 0.0, tail_contig=tail, score=score)
            if again == 2:
                continue
            for i in range(2 if again == 3 else 1):
                how = ('pipelined second pass', 'pipelined third pass', '', 'validating pass %d of two in flight' % (i + 1))[again] + \
                    ', tail_contig %d%s' % (tail, ', scored' if score else '')
                rec = dev.wait()
                how_it_ran(dev, et, how)
                compare(rec, orc, et, how, score)


def run_kind(dev, kind, motif, weights, k=6, skip=0, score=False, tails=None):
    dev.set_reference(E.ref_of(motif).arrays)
    if score:
        dev.set_mlp(*weights)
    for et in E.tables(kind, motif, k, skip):
        every_way(dev, et, weights, score=score, tails=tails)


@pytest.mark.parametrize('motif', MOTIFS)
def test_first_rows_of_reads_on_every_cut(dev, motif, weights):
    """Event 1: a read begins -2 .. +2 rows from every cut, behind a read that ends in an ordinary row, in a site row whose window
    the new read's first row closes (R6 / R8), and in filtered rows."""
    run_kind(dev, 'start', motif, weights)


@pytest.mark.parametrize('motif', MOTIFS)
def test_last_row_of_the_table_on_every_cut(dev, motif, weights):
    """Event 2: tables of cut + offset rows that end in an open window, which the next shard's first row closes (tail_contig 0)
    or nobody (-1)."""
    run_kind(dev, 'last', motif, weights, tails=(0, -1))


@pytest.mark.parametrize('motif', MOTIFS)
def test_closing_rows_on_every_cut(dev, motif, weights):
    """Event 3: a window's closing row -2 .. +2 rows from every cut, its closer directly behind it and behind one, two and
    three filtered rows."""
    run_kind(dev, 'close', motif, weights)


@pytest.mark.parametrize('motif', MOTIFS)
def test_first_site_rows_at_the_rounds_of_k0(dev, motif, weights):
    """Event 4: the first site row of a block 0, 1, 511, 512, 513, 1023, 1024 rows behind its first row, blocks of 512 and 513
    rows without one, a palindromic first site row of a reverse read (R5)."""
    run_kind(dev, 'f0', motif, weights)


@pytest.mark.parametrize('score', [False, True])
@pytest.mark.parametrize('motif', MOTIFS)
def test_window_lengths_at_the_look_back_steps(dev, motif, score, weights):
    """Event 5: windows of exactly 31 .. 66 rows whose closing row is a piece's / chunk's / tile's first row or the row behind
    it; scored: the walk inside the side stream's kernel finishes the long ones."""
    run_kind(dev, 'window', motif, weights, score=score)


@pytest.mark.parametrize('score', [False, True])
@pytest.mark.parametrize('motif', MOTIFS)
def test_slot_sizes_at_the_steps_of_the_pairwise_sum(dev, motif, score, weights):
    """Event 6: slots of exactly 7 .. 128 events, clear of the cuts and across them; 129 and 257 events: the pipelined pass is
    repeated."""
    run_kind(dev, 'slot', motif, weights, score=score)


@pytest.mark.parametrize('motif', MOTIFS)
def test_gaps_of_filtered_rows_across_every_cut(dev, motif, weights):
    """Event 7: 1 .. 65 filtered rows between a closing row in front of a cut and its closer behind it."""
    run_kind(dev, 'gap', motif, weights)


@pytest.mark.parametrize('motif', MOTIFS)
def test_a_violation_that_one_pair_of_rows_shows(dev, motif, weights):
    """Event 8: the table's FIRST pass, pipelined, and the first pass again after select_table(as_new): repeated (a row
    contradicts what its block was classified on) with the oracle's records; so is the pass behind each (flags complete)."""
    dev.set_reference(E.ref_of(motif).arrays)
    for et in E.tables('violation', motif):
        orc = oracle(et, -1, False, weights)
        slot = dev.upload_table_async(et.table, et.qual)
        for as_new in (False, True):
            if as_new:
                dev.select_table(slot, as_new=True)
            how = 'first pass%s' % (' (declared new)' if as_new else '')
            dev.run_async(et.k, et.skip, 0.0, score=False)
            rec = dev.wait()
            assert dev.last_pass_info()[1], '%s, %s: the pass was not repeated -- the pair %r was not seen' % (et.name, how, et.claims[0].more['pair'])
            compare(rec, orc, et, how, False)
            dev.run_async(et.k, et.skip, 0.0, score=False)
            compare(dev.wait(), orc, et, 'the pass behind the ' + how, False)
        dev.sync()


def test_more_closing_rows_in_a_tile_than_its_own_payload_slots(dev, weights):
    """Event 9: exactly 16, 17 and 18 closing rows in one tile of the scan under a sparse motif (a read across a short run of
    GATCGATC... in the genome): the 17th payload is the first that goes into a chunk from the shared counter."""
    run_kind(dev, 'tile', 'GATC' + E.RUNS, weights)


@pytest.mark.parametrize('motif', MOTIFS)
def test_more_name_blocks_than_the_tables_hold(dev, motif, weights):
    """Event 10: exactly 2, 3, 4 name blocks in a chunk of the scan; 16, 17, 18 in the staged rows of a piece of k1_fused and of
    k1_emit_runs."""
    run_kind(dev, 'blocks', motif, weights)


@pytest.mark.parametrize('motif', MOTIFS)
@pytest.mark.parametrize('k,skip', E.OTHER_K)
def test_starts_closing_rows_and_window_lengths_at_other_k(dev, k, skip, motif, weights):
    """The tables of events 1, 3 and 5 built again for k = 4 and 8 and for skip_thresh 1 (which row closes a window depends on
    both)."""
    for kind in E.OTHER_K_KINDS:
        run_kind(dev, kind, motif, weights, k=k, skip=skip)
