"""A first pass validates the event indices from the table's index-relation column (two bits per row, DevTable::xrel) where it
streamed the indices themselves.

(a) One violating pair of rows -- an equal index, an increase inside a decreasing block, a decrease inside an increasing one --
    whose second row sits on every cut the new load has: the unit edge (rows 7, 8, 9: bit 7 of a word, bit 0 of the next, bit 1),
    the stripe edge (511 .. 513: lane 0 of a stripe), the chunk edge (1023 .. 1025: stripe 0 of a chunk), the tile edge
    (2047 .. 2049: chunk 0 of a tile; once more at 3071 .. 3073 and 4095 .. 4097) and the table's last row, in tables of three
    tiles plus 1, 3 and 7 rows under a sparse and a one-base motif; the table goes up as bare arrays (the upload packs), with a
    maker's column and through pinned().  The pass must be repeated and every record must be the C oracle's.
(b) A block's first row stands in the "wrong" relation to the last row of the block in front of it, on the same cuts, in the
    middle of a unit, and with three and more blocks in one chunk: nothing may be seen -- the pass is not repeated.
(c) The column the device parser writes (kp_place) is the packer's on the index column it writes beside it, across waves and
    workgroups, with other lines between the rows.
(d) A slot that held another table's words: every word is written whole.
Runs on a real MI355X only."""
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
MOTIFS = ('GATC', 'A')
SIZES = (6145, 6147, 6151)          # three tiles of 2048 rows plus 1, 3 and 7: a last word of 1, 3 and 7 rows
CUTS = (8, 512, 1024, 2048, 3072, 4096)            # unit, stripe, chunk, tile; a chunk and a tile edge further on
KINDS = ('eq', 'inc', 'dec')
GENOME = 30000
# blocks of about 1100 rows: no chunk of 1024 rows holds more than two (the scan's fast path), every row of (a) lies four rows
# or more inside its block
STARTS_A = (0, 1100, 2200, 3300, 4400, 5500)
# (b): a block begins at cut + d (None); the others keep the blocks at two to a chunk, whichever d
STARTS_B = {8: (0, None, 1100, 2200, 3300, 4400, 5500), 512: (0, None, 1600, 2700, 3800, 4900, 6000),
            1024: (0, None, 2100, 3200, 4300, 5400), 2048: (0, 1000, None, 3100, 4200, 5300),
            3072: (0, 1000, 2040, None, 4120, 5200), 4096: (0, 1000, 2040, 3060, None, 5150)}
_cache = {}


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


def genome():
    from mcaller_amd import synth
    if 'codes' not in _cache:
        _cache['codes'] = synth.genome(length=GENOME, seed=3)
    return _cache['codes']


def ref_arrays(motif):
    from mcaller_amd import synth
    if ('ref', motif) not in _cache:
        _cache[('ref', motif)] = synth.SynthRef(genome(), motif=motif).device_arrays()
    return _cache[('ref', motif)]


def pool():
    """Synthetic reads of 1200 rows and more, made once: (table, qualities, [(first row, rows, index rises)])."""
    from mcaller_amd import synth
    if 'pool' not in _cache:
        table, qual = synth.make_table(60000, seed=41, codes=genome(), read_len=(1300, 1500))
        sb = table.seg_row_begin
        reads = [(int(sb[i]), int(sb[i + 1] - sb[i]), bool(table.event_idx[sb[i] + 1] > table.event_idx[sb[i]]))
                 for i in range(len(sb) - 2)]           # (the last read is cut off by the table's end)
        assert len(reads) > 20 and min(r[1] for r in reads) >= 1200
        _cache['pool'] = (table, qual, reads)
    return _cache['pool']


class Rows(object):
    """Blocks put together from the pool's reads, each cut to the rows it is given: columns that a test edits before it makes
    a Table of them."""

    def __init__(self, starts, n_rows, rises=None, first=0):
        table, qual, reads = pool()
        self.starts = list(starts)
        ends = self.starts[1:] + [n_rows]
        self.pos, self.evmu, self.idx, self.flags, self.qual = [], [], [], [], []
        at = first
        for bi, (a, b) in enumerate(zip(self.starts, ends)):
            want = None if rises is None else rises[bi % len(rises)]
            while want is not None and reads[at % len(reads)][2] != want:
                at += 1
            r0, n, _ = reads[at % len(reads)]
            assert 0 < b - a <= n
            self.pos.append(table.pos[r0:r0 + b - a])
            self.evmu.append(table.evmu[r0:r0 + b - a])
            self.idx.append(table.event_idx[r0:r0 + b - a])
            self.flags.append(table.flags[r0:r0 + b - a])
            self.qual.append(qual[at % len(reads)])
            at += 1
        self.pos, self.evmu = np.concatenate(self.pos), np.concatenate(self.evmu)
        self.idx, self.flags = np.concatenate(self.idx).copy(), np.concatenate(self.flags)
        self.qual = np.asarray(self.qual, dtype=np.float64)
        self.n_rows = n_rows

    def block_of(self, row):
        bi = int(np.searchsorted(self.starts, row, side='right')) - 1
        return self.starts[bi], (self.starts + [self.n_rows])[bi + 1]

    def rises(self, row):
        a, b = self.block_of(row)
        return b - a < 2 or bool(self.idx[a + 1] > self.idx[a])

    def table(self, way):
        """way 'bare': bare arrays, and the view names no column, so the upload call packs; 'maker': the maker hands a column
        over; 'pinned': through pinned()."""
        from mcaller_amd import _lib
        nb = len(self.starts)
        cls = bare_table if way == 'bare' else _lib.Table
        t = cls(self.pos, None, None, self.idx, self.flags, np.asarray(self.starts + [self.n_rows], dtype=np.int64),
                np.arange(nb, dtype=np.int32), np.zeros(nb, np.int32), nb, read_names=['read-%04d' % i for i in range(nb)],
                evmu=self.evmu, idx_rel_bits=None if way == 'bare' else _lib.pack_idx_rel(self.idx))
        return t.pinned() if way == 'pinned' else t


def orient(rows, target, kind):
    """'inc' wants a block whose indices fall, 'dec' one whose indices rise: the block around `target` mirrored if need be."""
    a, b = rows.block_of(target)
    if kind in ('inc', 'dec') and rows.rises(target) != (kind == 'dec'):
        rows.idx[a:b] = rows.idx[a:b][::-1].copy()


def rows_with_a_site(starts, n_rows, row, arrays, first, rises=None, kind=None):
    """Rows(...) from the first run of pool reads that gives the block around `row` (oriented for `kind`) a flush record: a
    block without a site row is not classified regular, and only what contradicts a regular block's classification repeats a
    pass."""
    bi = int(np.searchsorted(list(starts), row, side='right')) - 1
    for shift in range(60):
        rows = Rows(starts, n_rows, rises=rises, first=first + shift)
        orient(rows, row, kind)
        orc = H.oracle_records(rows.table('maker'), arrays, rows.qual, 6, 0, 0.0)
        if (np.asarray(orc.site_seg[:orc.n]) == bi).any():
            return rows
    raise AssertionError('no run of pool reads gives the block of row %d a record' % row)


def bare_table(*args, **kw):
    """A Table whose view names no relation column (NULL): mc_ctx_upload_table* pack it from event_idx."""
    from mcaller_amd import _lib

    class BareTable(_lib.Table):
        def view(self):
            v = super(BareTable, self).view()
            v.idx_rel_bits = None
            return v
    return BareTable(*args, **kw)


def violate(rows, target, kind):
    """One offending pair (target - 1, target), every other pair of the block as it was: 'eq' an equal index, 'inc' an increase
    inside a decreasing block, 'dec' a decrease inside an increasing block (the block's indices mirrored first if they run the
    other way; the rest of the block moves with the row, so that the pair behind it says what it said)."""
    a, b = rows.block_of(target)
    assert a + 2 <= target - 1 and target < b
    orient(rows, target, kind)
    up = rows.rises(target)
    if kind == 'eq':
        rows.idx[target:b] += -1 if up else 1
    else:
        rows.idx[target:b] += -2 if up else 2
    d = np.sign(np.diff(rows.idx[a:b].astype(np.int64)))
    want = {'eq': 0, 'inc': 1, 'dec': -1}[kind]
    assert d[target - a - 1] == want and (np.delete(d, target - a - 1) == (1 if up else -1)).all()


def passes(dev, table, qual, orc, repeated, what):
    """The synchronous first pass (the validating scan under both motifs); then, uploaded again, the pipelined first pass, the
    pass behind it, the first pass again after select_table(as_new=True) and the pass behind that."""
    def compare(rec, how):
        try:
            H.assert_records_equal(rec, orc, 6, prob_tol=1e-6)
        except AssertionError as e:
            raise AssertionError('%s, %s: %s' % (what, how, e))
    dev.upload_table(table)
    dev.set_read_quality(qual)
    compare(dev.extract(6, 0, 0.0), 'synchronous first pass')
    slot = dev.upload_table_async(table, qual)
    for as_new in (False, True):
        if as_new:
            dev.select_table(slot, as_new=True)
        how = 'first pass%s' % (' (declared new)' if as_new else '')
        dev.run_async(6, 0, 0.0)
        rec = dev.wait()
        assert dev.last_pass_info()[1] == repeated, '%s, %s: the pass was %srepeated' % (what, how, 'not ' if repeated else '')
        compare(rec, how)
        dev.run_async(6, 0, 0.0)
        compare(dev.wait(), 'the pass behind the ' + how)
    dev.sync()


def scored_oracle(table, qual, arrays, weights):
    orc = H.oracle_records(table, arrays, qual, 6, 0, 0.0)
    H.oracle_score(orc, table, qual, weights[0], weights[1], 6)
    return orc


@pytest.mark.parametrize('motif', MOTIFS)
@pytest.mark.parametrize('n_rows', SIZES)
def test_a_violating_pair_on_every_cut_of_the_relation_column(dev, n_rows, motif, weights):
    arrays = ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    targets = [c + d for c in CUTS for d in (-1, 0, 1)] + [n_rows - 1]
    n_rec = 0
    for ti, target in enumerate(targets):
        kind = KINDS[(ti + SIZES.index(n_rows) + MOTIFS.index(motif)) % 3]
        rows = rows_with_a_site(STARTS_A, n_rows, target, arrays, ti, kind=kind)
        violate(rows, target, kind)
        orc = scored_oracle(rows.table('maker'), rows.qual, arrays, weights)
        n_rec += orc.n
        for way in ('bare', 'maker', 'pinned'):
            passes(dev, rows.table(way), rows.qual, orc, True, '%d rows, %s, %s at (%d, %d), %s' % (n_rows, motif, kind, target - 1, target, way))
    assert n_rec > 12


def wrong_relations(rows):
    """Every block but the first begins with an index that stands to the last index of the block in front of it as no pair of
    its own rows does: equal, or the other way (in turn)."""
    for bi, a in enumerate(rows.starts[1:]):
        _, b = rows.block_of(a)
        up = rows.rises(a)
        delta = (0, -3 if up else 3)[bi % 2]
        rows.idx[a:b] += rows.idx[a - 1] + delta - rows.idx[a]
        rel = np.sign(int(rows.idx[a]) - int(rows.idx[a - 1]))
        assert rel == (0 if bi % 2 == 0 else (-1 if up else 1))


@pytest.mark.parametrize('motif', MOTIFS)
@pytest.mark.parametrize('n_rows', SIZES)
def test_a_blocks_first_row_is_not_compared_with_the_block_before(dev, n_rows, motif, weights):
    arrays = ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    n_rec = 0
    layouts = []
    for ci, c in enumerate(CUTS):
        d = (ci + SIZES.index(n_rows)) % 3 - 1          # (every cut gets -1, 0 and 1 over the three sizes: in the middle of a unit twice)
        layouts.append(('a block from row %d' % (c + d), [c + d if s is None else s for s in STARTS_B[c]], c + d))
    # three and more blocks in one chunk (rows from the third block's on are validated row by row from memory), blocks that
    # begin in the middle of a unit among them
    layouts.append(('five blocks in a chunk', [0, 150, 191, 230, 600, 1100, 2200, 3300, 4400, 5500], 230))
    layouts.append(('the table\'s last row a block', [0, 1100, 2200, 3300, 4400, 5500, n_rows - 1], 5500))
    for li, (name, starts, at) in enumerate(layouts):
        assert starts == sorted(set(starts)), starts
        # (the block that begins at `at` has a site row: it is classified regular, and a relation seen by mistake would repeat the pass)
        rows = rows_with_a_site(starts, n_rows, at, arrays, li, rises=(True, True, False, False, True, False))
        wrong_relations(rows)
        orc = scored_oracle(rows.table('maker'), rows.qual, arrays, weights)
        n_rec += orc.n
        for way in ('bare', 'maker', 'pinned'):
            passes(dev, rows.table(way), rows.qual, orc, False, '%d rows, %s, %s, %s' % (n_rows, motif, name, way))
    assert n_rec > 12


@pytest.mark.parametrize('motif', MOTIFS)
def test_a_violating_pair_in_a_chunks_third_block(dev, motif, weights):
    """... where the scan validates row by row from the index column itself: still seen, beside "wrong" relations at the
    blocks' first rows that are not."""
    arrays = ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    for ki, kind in enumerate(KINDS):
        target = (300, 450, 800)[ki]
        rows = rows_with_a_site([0, 150, 191, 230, 600, 1100, 2200, 3300, 4400, 5500], 6147, target, arrays, ki, kind=kind)
        wrong_relations(rows)
        violate(rows, target, kind)
        orc = scored_oracle(rows.table('maker'), rows.qual, arrays, weights)
        for way in ('bare', 'pinned'):
            passes(dev, rows.table(way), rows.qual, orc, True, '%s, %s in a third block, %s' % (motif, kind, way))


def shard_text(table, tmp_path, name, extra_lines):
    """The table as eventalign text with a header in front and lines of an unknown contig mixed in (row and line numbers differ,
    by another amount in every wave and workgroup of kp_place): the recipe of tests/test_gpu_model_n_bits.py."""
    from mcaller_amd import synth
    tsv = str(tmp_path / name)
    synth.write_tsv_native(table, genome(), tsv)
    lines = open(tsv, 'rb').read().split(b'\n')
    for at in sorted(extra_lines, reverse=True):
        lines.insert(at, b'elsewhere\t5\tAAAAAA\tr\tt\t7\t80.00\t1.0\t0.001\tAAAAAA\t81.00\t1.0\t0.1')
    lines.insert(0, b'contig\tposition\treference_kmer\tread_name\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length'
                    b'\tmodel_kmer\tmodel_mean\tmodel_stdv\tstandardized_level')
    open(tsv, 'wb').write(b'\n'.join(lines))
    return tsv


def parse_on_the_device(dev, tsv):
    from mcaller_amd import _lib
    host = _lib.parse_eventalign(tsv, 0, os.path.getsize(tsv), ['ecoli_syn'], exact_range=True)
    text = _lib.TextBlock(tsv, 0, os.path.getsize(tsv))
    slot = dev.parse_begin(text, ['ecoli_syn'], host.n_rows + 1024)
    t = dev.parse_end(slot, text)
    assert t is not None and t.n_rows == host.n_rows, getattr(dev, 'parse_fallback_reason', '')
    return host, t, slot, text


def pass_over_parsed(dev, host, t, qual_by_name, arrays, weights):
    q = np.asarray([qual_by_name[n] for n in t.read_names], dtype=np.float64)
    orc = scored_oracle(host, q, arrays, weights)
    dev.upload_table_async(t, q)
    dev.run_async(6, 0, 0.0)
    H.assert_records_equal(dev.wait(), orc, 6, prob_tol=1e-6)
    return orc


@pytest.mark.parametrize('n_rows', (700, 701, 707))
def test_the_device_parser_writes_the_column(dev, n_rows, tmp_path, weights):
    """A shard of a few hundred lines across the 64-line waves and 256-line workgroups of kp_place, reads whose indices rise and
    fall, equal neighbours on the waves' and workgroups' edges, other lines between the rows: the column is the packer's on the
    index column the parser wrote, and a pass over the table gives the oracle's records."""
    from mcaller_amd import _lib, synth
    table, qual = synth.make_table(n_rows, seed=21, codes=genome(), read_len=(150, 400))
    idx = table.event_idx
    for a in (5, 62, 63, 64, 250, 254, 255, 256, 257, 300, 509, 510, 511, 512, n_rows - 2, n_rows - 1):
        if not table.flags[a] & 4:
            idx[a] = idx[a - 1]
    tsv = shard_text(table, tmp_path, 'x.tsv', (3, 4, 61, 70, 200, 255, 256, 300, 511, 650))
    host, t, slot, text = parse_on_the_device(dev, tsv)
    assert t.unknown == ['contig'] + ['elsewhere'] * 10 and np.array_equal(host.event_idx, table.event_idx)
    pos, evmu, got_idx, flags = dev.fetch_columns(slot, t.n_rows)
    assert np.array_equal(got_idx, host.event_idx)
    rel = dev.fetch_idx_rel_bits(slot, t.n_rows)
    want = _lib.pack_idx_rel(got_idx)
    assert np.array_equal(rel, want), np.flatnonzero(rel != want)
    assert np.array_equal(host.idx_rel_bits, want)
    inc = int(np.unpackbits((want & 0xFF).astype(np.uint8)).sum())
    dec = int(np.unpackbits((want >> 8).astype(np.uint8)).sum())
    assert inc > 50 and dec > 50 and 10 <= n_rows - 1 - inc - dec          # (all three relations among the rows)
    arrays = ref_arrays('A')
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    orc = pass_over_parsed(dev, host, t, dict(zip(table.read_names, qual)), arrays, weights)
    assert orc.n > 20


def test_a_slot_that_held_another_tables_words(dev, tmp_path, weights):
    """Every index below the one before it, parsed into a slot; then a shard of the same size whose indices all rise into the
    same slot: every word of the column is written, not ORed into what was there -- no "less than" bit is left, and the records
    are the oracle's."""
    from mcaller_amd import _lib, synth
    table, qual = synth.make_table(3000, seed=22, codes=genome(), read_len=(150, 400))
    falling = (70000 - 2 * np.arange(3000)).astype(np.int32)
    rising = (1000 + 2 * np.arange(3000)).astype(np.int32)
    slots = []
    for name, idx in (('falling.tsv', falling), ('rising.tsv', rising)):
        tab = _lib.Table(table.pos, None, None, idx, table.flags, table.seg_row_begin, table.seg_read, table.seg_contig,
                         table.n_reads, read_names=table.read_names, evmu=table.evmu)
        tsv = shard_text(tab, tmp_path, name, (7, 300, 1000))
        host, t, slot, text = parse_on_the_device(dev, tsv)
        slots.append(slot)
        rel = dev.fetch_idx_rel_bits(slot, t.n_rows)
        assert np.array_equal(host.event_idx, idx) and np.array_equal(rel, _lib.pack_idx_rel(idx))
        if name == 'falling.tsv':
            assert rel[0] == 0xFE00 and (rel[1:] == 0xFF00).all()
            dev.parse_abandon(slot)
    assert slots[0] == slots[1], 'the second shard went to another slot: %r' % slots
    assert rel[0] == 0x00FE and (rel[1:] == 0x00FF).all()
    arrays = ref_arrays('A')
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    orc = pass_over_parsed(dev, host, t, dict(zip(table.read_names, qual)), arrays, weights)
    assert orc.n > 100
