"""A first pass under a sparse motif validates every row from the columns the table's maker writes with the positions -- the unit
summaries (DevTable::unit_pp) and the position-relation column (DevTable::prel) -- and the index-relation column, and filters on
the summaries (k1_scan<64, SCAN_VALIDATE_SUMMARY>); every later pass reads the summaries alone.

(a) The columns fetched from the slot are numpy's (tests/test_pos_rel_bits.py) on the position column beside them: after an
    upload of bare arrays, after pinned() (k_unit_columns), after the device parser (kp_place: rows across waves and workgroups,
    other lines between them), and in a slot that held a longer table with other bits.
(b) One violating pair -- a position below the one before it, a position 0 -- with its second row on the unit, stripe, chunk and
    tile edges and on the table's last row (the cuts of tests/test_gpu_idx_rel_bits.py, whose blocks and reads these tests use):
    the first pass is repeated, and the records are the C oracle's on the synchronous pass, the first pass, the first pass
    declared new and the pass behind each.  GATC takes the new instance and the summary instance behind it; a one-base motif
    takes the instances it took.
(c) A block whose first row lies below the last row of the block in front of it, on the same cuts and in the middle of a unit:
    nothing is seen, nothing repeated.
(d) A violating pair in a chunk's third block and in units cut by a block's ends, which read the columns from memory.
Runs on a real MI355X only."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_idx_rel_bits as X
from tests.test_pos_rel_bits import pos_rel_bits, unit_summaries

pytestmark = pytest.mark.gpu
dev = X.dev
weights = X.weights
SIZES, CUTS, STARTS_A, STARTS_B = X.SIZES, X.CUTS, X.STARTS_A, X.STARTS_B
KINDS = ('pdec', 'pos0')
# mc_ctx_last_scan_mode: what (first pass, later pass) stream under a sparse and under a one-base motif
MODES = {'GATC': (3, 2), 'A': (0, 1)}


def check_columns(dev, slot, pos, what):
    n = len(pos)
    rel, pp = dev.fetch_pos_rel_bits(slot, n), dev.fetch_unit_summaries(slot, n)
    want = pos_rel_bits(pos)
    assert np.array_equal(rel, want), '%s: words %r' % (what, np.flatnonzero(rel != want)[:8])
    first, last = unit_summaries(pos)
    assert np.array_equal(pp[:, 0], first), '%s: first positions of units %r' % (what, np.flatnonzero(pp[:, 0] != first)[:8])
    assert np.array_equal(pp[:n // 8, 1], last), '%s: last positions of units %r' % (what, np.flatnonzero(pp[:n // 8, 1] != last)[:8])
    return want


def violate(rows, target, kind):
    """One offending pair (target - 1, target) inside a block: the position of `target` one below its predecessor's, or 0."""
    a, b = rows.block_of(target)
    assert a <= target - 1 and target < b and rows.pos[target - 1] >= 2
    rows.pos[target] = rows.pos[target - 1] - 1 if kind == 'pdec' else 0
    d = np.diff(rows.pos[a:b].astype(np.int64))
    assert d[target - a - 1] < 0 and (np.delete(d, target - a - 1) >= 0).all()


def passes(dev, table, qual, orc, repeated, motif, what):
    """The synchronous first pass; then, uploaded again, the pipelined first pass, the pass behind it, the first pass again after
    select_table(as_new=True) and the pass behind that -- each with the scan instance it has to take."""
    def compare(rec, how):
        try:
            H.assert_records_equal(rec, orc, 6, prob_tol=1e-6)
        except AssertionError as e:
            raise AssertionError('%s, %s: %s' % (what, how, e))
    first_mode, later_mode = MODES[motif]
    dev.upload_table(table)
    dev.set_read_quality(qual)
    compare(dev.extract(6, 0, 0.0), 'synchronous first pass')
    slot = dev.upload_table_async(table, qual)
    for as_new in (False, True):
        if as_new:
            dev.select_table(slot, as_new=True)
        how = 'first pass%s' % (' (declared new)' if as_new else '')
        dev.run_async(6, 0, 0.0)
        assert dev.last_scan_mode() == first_mode, '%s, %s: scan mode %d' % (what, how, dev.last_scan_mode())
        rec = dev.wait()
        assert dev.last_pass_info()[1] == repeated, '%s, %s: the pass was %srepeated' % (what, how, 'not ' if repeated else '')
        compare(rec, how)
        dev.run_async(6, 0, 0.0)
        assert dev.last_scan_mode() == later_mode, '%s, the pass behind the %s: scan mode %d' % (what, how, dev.last_scan_mode())
        compare(dev.wait(), 'the pass behind the ' + how)
    dev.sync()
    return slot


def table_of(rows, ti):
    return rows.table(('maker', 'pinned')[ti % 2])


@pytest.mark.parametrize('n_rows', SIZES)
def test_the_columns_after_an_upload(dev, n_rows):
    """Bare arrays and pinned(): k_unit_columns behind the position column's transfer.  Decreases and zeros on the edges of
    its threads (four rows), units, waves (256 rows) and workgroups (1024 rows), in the table's first and last rows."""
    rows = X.Rows(STARTS_A, n_rows)
    for at in (0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2048, 4095, 4096, n_rows - 2, n_rows - 1):
        rows.pos[at] = 0 if at % 3 == 0 else max(int(rows.pos[at - 1]) - 1, 1)
    want = None
    for way in ('bare', 'pinned'):
        slot = dev.upload_table_async(rows.table(way), rows.qual)
        pos = dev.fetch_columns(slot, n_rows)[0]
        assert np.array_equal(pos, rows.pos)
        want = check_columns(dev, slot, pos, '%d rows, %s' % (n_rows, way))
        dev.sync()
    dec = int(np.unpackbits((want & 0xFF).astype(np.uint8)).sum())
    zero = int(np.unpackbits((want >> 8).astype(np.uint8)).sum())
    assert dec >= 8 and zero >= 6


def test_a_slot_that_held_a_longer_table(dev):
    """Every position below the one before it and 0 in every other row, 6151 rows; then 6145 rising rows into the same slot:
    every word of [0, ceil(n / 8)) is the new table's -- the last one with a single row's bits."""
    long_rows, short_rows = X.Rows(STARTS_A, 6151), X.Rows(STARTS_A, 6145)
    long_rows.pos[:] = 2 * (7000 - np.arange(6151))
    long_rows.pos[1::2] = 0
    short_rows.pos[:] = 5 + np.arange(6145)
    slot0 = dev.upload_table_async(long_rows.table('bare'), long_rows.qual)
    rel = check_columns(dev, slot0, long_rows.pos, 'the longer table')
    assert rel[0] == 0xAAAA and (rel[1:-1] == 0xAAAA).all() and rel[-1] == 0x2A2A
    dev.sync()
    for _ in range(16):                                 # (the slots are taken in turn)
        slot = dev.upload_table_async(short_rows.table('bare'), short_rows.qual)
        dev.sync()
        if slot == slot0:
            break
    assert slot == slot0, 'the shorter table never went to slot %d' % slot0
    rel = check_columns(dev, slot, short_rows.pos, 'the shorter table')
    assert len(rel) == 769 and not rel.any()


@pytest.mark.parametrize('n_rows', (700, 701, 707))
def test_the_device_parser_writes_the_columns(dev, n_rows, tmp_path, weights):
    """A shard of a few hundred lines across the 64-line waves and 256-line workgroups of kp_place, other lines between the
    rows, decreases and zeros on the waves' and workgroups' edges and in the last rows; then a first pass over it."""
    from mcaller_amd import synth
    table, qual = synth.make_table(n_rows, seed=21, codes=X.genome(), read_len=(150, 400))
    for a in (5, 62, 63, 64, 250, 254, 255, 256, 257, 300, 509, 510, 511, 512, n_rows - 2, n_rows - 1):
        if not table.flags[a] & 4:
            table.pos[a] = 0 if a % 3 == 0 else max(int(table.pos[a - 1]) - 1, 1)
    tsv = X.shard_text(table, tmp_path, 'p.tsv', (3, 4, 61, 70, 200, 255, 256, 300, 511, 650))
    host, t, slot, text = X.parse_on_the_device(dev, tsv)
    assert np.array_equal(host.pos, table.pos)
    pos = dev.fetch_columns(slot, t.n_rows)[0]
    assert np.array_equal(pos, host.pos)
    want = check_columns(dev, slot, pos, '%d rows parsed on the device' % n_rows)
    assert int(np.unpackbits((want & 0xFF).astype(np.uint8)).sum()) >= 8 and int(np.unpackbits((want >> 8).astype(np.uint8)).sum()) >= 3
    arrays = X.ref_arrays('GATC')
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    q = np.asarray([dict(zip(table.read_names, qual))[n] for n in t.read_names], dtype=np.float64)
    orc = X.scored_oracle(host, q, arrays, weights)
    dev.upload_table_async(t, q)
    for mode in MODES['GATC']:
        dev.run_async(6, 0, 0.0)
        assert dev.last_scan_mode() == mode
        H.assert_records_equal(dev.wait(), orc, 6, prob_tol=1e-6)
    assert orc.n > 0


def test_a_slot_the_device_parser_fills_again(dev, tmp_path):
    """3000 rows whose positions all fall, parsed into a slot; then 2995 rows whose positions all rise into the same slot: the
    words are stored whole, not ORed into what was there."""
    from mcaller_amd import _lib, synth
    slots = []
    for name, n, pos in (('falling.tsv', 3000, 2 * (4000 - np.arange(3000))), ('rising.tsv', 2995, 5 + np.arange(2995))):
        cut, _ = synth.make_table(n, seed=22, codes=X.genome(), read_len=(150, 400))
        tab = _lib.Table(pos.astype(np.int32), None, None, cut.event_idx, cut.flags, cut.seg_row_begin, cut.seg_read, cut.seg_contig,
                         cut.n_reads, read_names=cut.read_names, evmu=cut.evmu)
        tsv = X.shard_text(tab, tmp_path, name, (7, 300, 1000))
        host, t, slot, text = X.parse_on_the_device(dev, tsv)
        slots.append(slot)
        got = dev.fetch_columns(slot, t.n_rows)[0]
        assert np.array_equal(got, pos)
        rel = check_columns(dev, slot, got, name)
        if name == 'falling.tsv':
            assert rel[0] == 0x00FE and (rel[1:] == 0x00FF).all()
        dev.parse_abandon(slot)
    assert slots[0] == slots[1], 'the second shard went to another slot: %r' % slots
    assert len(rel) == 375 and not rel.any()


@pytest.mark.parametrize('motif', X.MOTIFS)
@pytest.mark.parametrize('n_rows', SIZES)
def test_a_violating_pair_on_every_cut(dev, n_rows, motif, weights):
    arrays = X.ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    targets = [c + d for c in CUTS for d in (-1, 0, 1)] + [n_rows - 1]
    n_rec = 0
    for ti, target in enumerate(targets):
        for ki, kind in enumerate(KINDS):
            rows = X.rows_with_a_site(STARTS_A, n_rows, target, arrays, ti)
            violate(rows, target, kind)
            orc = X.scored_oracle(rows.table('maker'), rows.qual, arrays, weights)
            n_rec += orc.n
            passes(dev, table_of(rows, ti + ki + SIZES.index(n_rows)), rows.qual, orc, True, motif,
                   '%d rows, %s, %s at (%d, %d)' % (n_rows, motif, kind, target - 1, target))
    assert n_rec > 12


def rows_with_a_low_first_row(starts, n_rows, at, arrays, first):
    """Rows(...) from the first run of pool reads that gives the block that begins at `at` a flush record (see
    X.rows_with_a_site) and a first position below the last position of the block in front of it."""
    bi = list(starts).index(at)
    for shift in range(200):
        rows = X.Rows(starts, n_rows, first=first + shift)
        if not rows.pos[at] < rows.pos[at - 1]:
            continue
        orc = H.oracle_records(rows.table('maker'), arrays, rows.qual, 6, 0, 0.0)
        if (np.asarray(orc.site_seg[:orc.n]) == bi).any():
            return rows
    raise AssertionError('no run of pool reads gives the block at row %d a record and a first row below row %d' % (at, at - 1))


@pytest.mark.parametrize('motif', X.MOTIFS)
@pytest.mark.parametrize('n_rows', SIZES)
def test_a_blocks_first_row_below_the_block_before(dev, n_rows, motif, weights):
    arrays = X.ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    n_rec = 0
    for ci, c in enumerate(CUTS):
        d = (ci + SIZES.index(n_rows)) % 3 - 1          # (every cut gets -1, 0 and 1 over the three sizes: in the middle of a unit twice)
        starts = [c + d if s is None else s for s in STARTS_B[c]]
        rows = rows_with_a_low_first_row(starts, n_rows, c + d, arrays, ci)
        assert (pos_rel_bits(rows.pos)[(c + d) >> 3] >> ((c + d) & 7)) & 1       # (the column says "below": nobody may count it)
        orc = X.scored_oracle(rows.table('maker'), rows.qual, arrays, weights)
        n_rec += orc.n
        passes(dev, table_of(rows, ci), rows.qual, orc, False, motif, '%d rows, %s, a block from row %d' % (n_rows, motif, c + d))
    assert n_rec > 12


@pytest.mark.parametrize('motif', X.MOTIFS)
def test_a_violating_pair_in_a_third_block_and_in_a_cut_unit(dev, motif, weights):
    """... where the scan validates row by row from the position column itself."""
    arrays = X.ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    crowded = [0, 150, 191, 230, 600, 1100, 2200, 3300, 4400, 5500]
    # a chunk's third block and beyond | the unit of rows 1096 .. 1103, cut by the blocks' boundary at row 1100: the rows in
    # front of it, the rows behind it | the first unit of a block that begins on a unit's edge (its first row has no predecessor)
    cases = [(crowded, 300), (crowded, 450), (crowded, 800), (list(STARTS_A), 1098), (list(STARTS_A), 1102), (list(STARTS_A), 1103),
             ([0, 1104, 2200, 3300, 4400, 5500], 1105), ([0, 1104, 2200, 3300, 4400, 5500], 1111)]
    for ci, (starts, target) in enumerate(cases):
        kind = KINDS[ci % 2]
        rows = X.rows_with_a_site(starts, 6147, target, arrays, ci)
        violate(rows, target, kind)
        orc = X.scored_oracle(rows.table('maker'), rows.qual, arrays, weights)
        passes(dev, table_of(rows, ci), rows.qual, orc, True, motif, '%s, %s at row %d of %r' % (motif, kind, target, starts))
