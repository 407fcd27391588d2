"""The scan reads a table's model-N bit column (one bit per row, DevTable::nbits) where it read the flag bytes: 'N' rows placed on
every cut the new load has -- the byte / lane edge (rows 7, 8, 9), the stripe edge (511 .. 513), the chunk edge (1023 .. 1025), the
tile edge (2047 .. 2049), the table's last two rows, the rows behind site rows -- in runs of one, two and three, in tables of
three tiles plus 1, 3 and 7 rows, under a sparse and a one-base motif, in every way tests/test_gpu_edges.py scans a table, against
the C oracle: integers and slot means bit for bit, probabilities as test_gpu_edges.py compares them.  And the column the device
parser writes (kp_place) against the packed flag column it writes beside it, also into a slot that held another table's bits.
Runs on a real MI355X only."""
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
MOTIFS = ('GATC', 'A')
SIZES = (6145, 6147, 6151)          # three tiles of 2048 rows plus 1, 3 and 7: n_rows % 8 of 1, 3 and 7
CUTS = (8, 512, 1024, 2048, 2560, 3072, 4096)      # byte / lane, stripe, chunk, tile; a stripe, chunk and tile edge further on (the
                                                    # third tile's end is the table's: its last rows get a run of their own)
GENOME = 30000
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


def packed(flags):
    return np.packbits((np.asarray(flags, dtype=np.uint8) >> 1) & 1, bitorder='little')


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


def base_table(n_rows):
    """A synthetic table of short reads none of which begins within four rows of a cut or of the table's end (the 'N' runs below
    stay inside reads).  Made once per size and left as it is."""
    from mcaller_amd import synth
    if ('base', n_rows) not in _cache:
        for seed in range(100, 200):
            table, qual = synth.make_table(n_rows, seed=seed, codes=genome(), read_len=(300, 900))
            starts = table.seg_row_begin[1:-1]
            if all(((starts < c - 4) | (starts >= c + 5)).all() for c in CUTS + (n_rows,)):
                break
        else:
            raise AssertionError('no seed keeps the reads\' first rows clear of the cuts')
        _cache[('base', n_rows)] = (table, qual)
    return _cache[('base', n_rows)]


def site_closers(n_rows, motif):
    """Rows behind site rows: closing rows of a few of the base table's windows, spread over the table (from the oracle)."""
    if ('closers', n_rows, motif) not in _cache:
        table, qual = base_table(n_rows)
        orc = H.oracle_records(table, ref_arrays(motif), qual, 6, 0, 0.0)
        rows = np.unique(np.asarray(orc.close_row[:orc.n], dtype=np.int64))
        rows = rows[(rows > 0) & (rows < n_rows - 8)]
        assert len(rows) >= 4, 'the base table closes too few windows under %s' % motif
        _cache[('closers', n_rows, motif)] = rows[::max(1, len(rows) // 8)][:8]
    return _cache[('closers', n_rows, motif)]


def n_table(n_rows, motif, run, variant):
    """The base table with runs of `run` 'N' rows: one across every cut, beginning run .. -1 rows in front of it (which, depends on
    the cut and the variant: all of them over the run + 2 variants), one at the table's end (its last row, or the one before),
    and one directly behind each of a few site rows."""
    from mcaller_amd import _lib
    table, qual = base_table(n_rows)
    fl = table.flags.copy()
    taken = np.zeros(n_rows, dtype=bool)

    def put(a):
        a, b = max(int(a), 1), min(int(a) + run, n_rows)
        if taken[max(a - 2, 0):b + 2].any() or (fl[a:b] & _lib.F_SEG_START).any():
            return False
        fl[a:b] |= _lib.F_MODEL_N
        fl[a:b] &= np.uint8(0xFF ^ _lib.F_KMER_EQ)
        taken[a:b] = True
        return True
    for i, c in enumerate(CUTS):
        assert put(c - run + (i + variant) % (run + 2)), (n_rows, run, variant, c)
    assert put(n_rows - (variant % 2) - run)
    assert sum(put(r) for r in site_closers(n_rows, motif)) >= 2
    t = _lib.Table(table.pos, None, None, table.event_idx, fl, table.seg_row_begin, table.seg_read, table.seg_contig, table.n_reads,
                   read_names=table.read_names, evmu=table.evmu)
    return t, qual


def every_way(dev, table, qual, arrays, weights, what):
    """tests/test_gpu_edges.py's sequence: synchronous first pass, pipelined second and third pass, and, declared new, two
    validating passes in flight."""
    orc = H.oracle_records(table, arrays, qual, 6, 0, 0.0)
    H.oracle_score(orc, table, qual, weights[0], weights[1], 6)
    dev.upload_table(table)
    dev.set_read_quality(qual)
    slot = dev.current_slot()

    def compare(rec, how):
        try:
            H.assert_records_equal(rec, orc, 6, prob_tol=1e-6)
        except AssertionError as e:
            raise AssertionError('%s, %s: %s' % (what, how, e))
    compare(dev.extract(6, 0, 0.0), 'synchronous first pass')
    for again in range(4):
        if again == 2:
            dev.select_table(slot, as_new=True)
        dev.run_async(6, 0, 0.0)
        if again == 2:
            continue
        for i in range(2 if again == 3 else 1):
            compare(dev.wait(), ('pipelined second pass', 'pipelined third pass', '', 'validating pass %d of two in flight' % (i + 1))[again])
    return orc


@pytest.mark.parametrize('motif', MOTIFS)
@pytest.mark.parametrize('n_rows', SIZES)
def test_n_rows_on_every_cut_of_the_bit_column(dev, n_rows, motif, weights):
    arrays = ref_arrays(motif)
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    n_rec = 0
    for run in (1, 2, 3):
        for variant in range(run + 2):
            table, qual = n_table(n_rows, motif, run, variant)
            for c in CUTS:          # (what the table is for: every cut has an 'N' row on one side of it or on both)
                assert (table.flags[c - run:c + 2] & 2).any()
            n_rec += every_way(dev, table, qual, arrays, weights, '%d rows, %s, runs of %d, variant %d' % (n_rows, motif, run, variant)).n
    assert n_rec > 12


def shard_text(table, tmp_path, name, extra_lines):
    """The table as eventalign text with a header in front and lines of an unknown contig mixed in (row and line numbers differ,
    by another amount in every wave and workgroup of kp_place)."""
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
    orc = H.oracle_records(host, arrays, q, 6, 0, 0.0)
    H.oracle_score(orc, host, q, weights[0], weights[1], 6)
    dev.upload_table_async(t, q)
    dev.run_async(6, 0, 0.0)
    H.assert_records_equal(dev.wait(), orc, 6, prob_tol=1e-6)
    return orc


@pytest.mark.parametrize('n_rows', (700, 701, 707))
def test_the_device_parser_writes_the_column(dev, n_rows, tmp_path, weights):
    """A shard of a few hundred lines across the 64-line waves and 256-line workgroups of kp_place, 'N' rows among them, other
    lines between the rows: the bit column is the packed flag column, and a pass over the table gives the oracle's records."""
    from mcaller_amd import synth
    table, qual = synth.make_table(n_rows, seed=21, codes=genome(), read_len=(150, 400))
    fl = table.flags
    for a in (5, 62, 63, 64, 250, 254, 255, 256, 257, 300, 509, 510, 511, 512, n_rows - 2, n_rows - 1):
        if not fl[a] & 4:
            fl[a] = (fl[a] | 2) & 0xFE
    tsv = shard_text(table, tmp_path, 'n.tsv', (3, 4, 61, 70, 200, 255, 256, 300, 511, 650))
    host, t, slot, text = parse_on_the_device(dev, tsv)
    assert t.unknown == ['contig'] + ['elsewhere'] * 10 and np.array_equal(host.flags, table.flags)
    pos, evmu, idx, flags = dev.fetch_columns(slot, t.n_rows)
    assert np.array_equal(flags, host.flags) and int((flags & 2 != 0).sum()) > 20
    bits = dev.fetch_model_n_bits(slot, t.n_rows)
    assert np.array_equal(bits, packed(flags)), np.flatnonzero(bits != packed(flags))
    arrays = ref_arrays('A')
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    orc = pass_over_parsed(dev, host, t, dict(zip(table.read_names, qual)), arrays, weights)
    assert orc.n > 20


def test_a_slot_that_held_another_tables_bits(dev, tmp_path, weights):
    """Most rows 'N', parsed into a slot; then a shard of the same size without an 'N' row into the same slot: every byte of the
    column is written, not ORed into what was there -- no bit is left, and the records are the oracle's."""
    from mcaller_amd import _lib, synth
    table, qual = synth.make_table(3000, seed=22, codes=genome(), read_len=(150, 400))
    clean = table.flags & np.uint8(0xFF ^ _lib.F_MODEL_N)
    rng = np.random.default_rng(5)
    mostly = np.where((rng.random(3000) < 0.9) & ((clean & _lib.F_SEG_START) == 0), (clean | _lib.F_MODEL_N) & 0xFE, clean).astype(np.uint8)
    slots = []
    for name, flags in (('mostly_n.tsv', mostly), ('clean.tsv', clean)):
        tab = _lib.Table(table.pos, None, None, table.event_idx, flags, table.seg_row_begin, table.seg_read, table.seg_contig,
                         table.n_reads, read_names=table.read_names, evmu=table.evmu)
        tsv = shard_text(tab, tmp_path, name, (7, 300, 1000))
        host, t, slot, text = parse_on_the_device(dev, tsv)
        slots.append(slot)
        bits = dev.fetch_model_n_bits(slot, t.n_rows)
        assert np.array_equal(host.flags, flags) and np.array_equal(bits, packed(flags))
        if name == 'mostly_n.tsv':
            assert int(np.unpackbits(bits).sum()) > 2000
            dev.parse_abandon(slot)
    assert slots[0] == slots[1], 'the second shard went to another slot: %r' % slots
    assert not bits.any()
    arrays = ref_arrays('A')
    dev.set_reference(arrays)
    dev.set_mlp(*weights)
    orc = pass_over_parsed(dev, host, t, dict(zip(table.read_names, qual)), arrays, weights)
    assert orc.n > 100
