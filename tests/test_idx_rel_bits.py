"""The index-relation column (mc_table_view.idx_rel_bits: a uint16 per unit of eight rows, row r = 8u + e: bit e of word u is
event_idx[r] > event_idx[r - 1], bit 8 + e is event_idx[r] < event_idx[r - 1], neither means equal; row 0 and the bits beyond the
last row are 0) on the host: the native packer against a numpy restatement, and every maker and carrier of a host table -- the
parser, the synthetic table, pinned(), view(), slice_segments() -- against the packer on the table's own index column.  No GPU."""
import ctypes as C

import numpy as np
import pytest

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def rel_numpy(idx):
    """np.sign(np.diff(idx)) as two bit planes, a uint16 per eight rows (the differences in 64 bits: INT32_MIN beside INT32_MAX)."""
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx)
    sign = np.zeros(n, dtype=np.int64)
    sign[1:] = np.sign(np.diff(idx))
    inc = np.packbits(sign > 0, bitorder='little').astype(np.uint16)
    dec = np.packbits(sign < 0, bitorder='little').astype(np.uint16)
    return (inc | (dec << 8)).astype(np.uint16)


def wild_indices(n_rows, seed):
    """Runs up, runs down, equal neighbours, and the ends of the 32-bit range side by side."""
    rng = np.random.default_rng(seed)
    idx = np.cumsum(rng.integers(-2, 3, size=n_rows)).astype(np.int32)
    edge = np.array([I32_MIN, I32_MAX, I32_MAX, I32_MIN, I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX, 0, I32_MIN, 0, I32_MAX], dtype=np.int32)
    for at in (0, 5, 60, 3000, n_rows - len(edge)):
        if 0 <= at and at + len(edge) <= n_rows:
            idx[at:at + len(edge)] = edge
    return idx


def small_table(seg_begin, seed, maker_column):
    from mcaller_amd import _lib
    n = int(seg_begin[-1])
    idx = wild_indices(n, seed)
    ns = len(seg_begin) - 1
    return _lib.Table(np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), idx, np.zeros(n, np.uint8),
                      np.asarray(seg_begin, dtype=np.int64), np.arange(ns, dtype=np.int32), np.zeros(ns, np.int32), ns,
                      idx_rel_bits=_lib.pack_idx_rel(idx) if maker_column else None)


@pytest.mark.parametrize('n_rows', [0, 1, 7, 8, 9, 6145, 6147, 6151])
def test_pack_idx_rel_is_the_sign_of_numpys_diff(n_rows):
    from mcaller_amd import _lib
    idx = wild_indices(n_rows, 2000 + n_rows)
    n_words = (n_rows + 7) // 8
    out = np.full(n_words + 8, 0xA5A5, dtype=np.uint16)       # (every word of the column is written, none behind it)
    _lib.lib().mc_pack_idx_rel(idx.ctypes.data_as(C.c_void_p), n_rows, out.ctypes.data_as(C.c_void_p))
    want = rel_numpy(idx)
    assert len(want) == n_words and np.array_equal(out[:n_words], want) and (out[n_words:] == 0xA5A5).all()
    assert np.array_equal(_lib.pack_idx_rel(idx), want)
    if n_rows:
        assert not want[0] & 0x0101                             # row 0 has no row before it
        assert not (int(want[-1]) >> 8 | int(want[-1])) & 0xFF & ~((1 << ((n_rows - 1) % 8 + 1)) - 1)     # nothing beyond the last row
    if n_rows >= 12:                                            # INT32_MIN -> INT32_MAX -> INT32_MAX -> INT32_MIN at rows 0 .. 3
        assert want[0] & 0x0F0F == 0x0802


@pytest.mark.parametrize('maker_column', [False, True])
def test_slice_segments_at_every_offset_inside_a_word(maker_column):
    """Segments that start at rows with r0 % 8 of 0, 1 and 7 (and end inside a word): the slice's column is the packer's on the
    slice's indices -- its first row has no row before it any more."""
    from mcaller_amd import _lib
    seg_begin = [0, 16, 33, 47, 64, 81, 103, 128, 131]
    t = small_table(seg_begin, 7, maker_column)
    assert np.array_equal(t.idx_rel_bits, rel_numpy(t.event_idx))
    seen = set()
    for s0 in range(len(seg_begin) - 1):
        for s1 in range(s0 + 1, len(seg_begin)):
            sub = t.slice_segments(s0, s1)
            assert np.array_equal(sub.event_idx, t.event_idx[seg_begin[s0]:seg_begin[s1]])
            assert np.array_equal(sub.idx_rel_bits, _lib.pack_idx_rel(sub.event_idx)), (s0, s1)
            assert np.array_equal(sub.idx_rel_bits, rel_numpy(sub.event_idx)), (s0, s1)
            assert (sub._idx_rel_bits is not None) == (maker_column and seg_begin[s0] % 8 == 0)
            seen.add(seg_begin[s0] % 8)
    assert {0, 1, 7} <= seen
    assert np.array_equal(t.idx_rel_bits, rel_numpy(t.event_idx))      # (slicing left the table's own column alone)


@pytest.mark.parametrize('maker_column', [False, True])
def test_pinned_and_view_carry_the_column(maker_column):
    t = small_table([0, 10, 21], 11, maker_column)
    want = rel_numpy(t.event_idx)
    p = t.pinned()
    assert p._idx_rel_bits is not None and np.array_equal(p.idx_rel_bits, want)
    assert p.idx_rel_bits.ctypes.data != t.idx_rel_bits.ctypes.data     # (no alias of the source)
    for tab in (t, p):
        v = tab.view()
        assert v.idx_rel_bits and v.event_idx
        got = np.frombuffer((C.c_char * (2 * len(want))).from_address(v.idx_rel_bits), dtype=np.uint16)
        assert np.array_equal(got, want)
    assert p.view().idx_rel_bits == p.idx_rel_bits.ctypes.data          # (the pinned block itself: nothing is packed per upload)


def test_bare_arrays_are_packed_from_the_indices_as_they_are():
    """A table made from bare arrays whose indices are edited afterwards hands out the edited column."""
    t = small_table([0, 40], 13, False)
    t.event_idx[:] = np.arange(40)
    t.event_idx[9] = t.event_idx[8]
    t.event_idx[17] = 3
    want = rel_numpy(t.event_idx)
    assert np.array_equal(t.idx_rel_bits, want)
    assert want[0] == 0x00FE and want[1] == 0x00FD and want[2] == 0x02FD


def idx_tsv(n_rows, seed):
    """eventalign lines of three reads on one contig whose event indices run up, down and stand still; a header and lines of an
    unknown contig between them."""
    idx = np.cumsum(np.random.default_rng(seed).integers(-1, 2, size=n_rows)) + 5000
    lines = ['contig\tposition\treference_kmer\tread_name\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\tmodel_kmer\tmodel_mean\tmodel_stdv\tstandardized_level']
    for i in range(n_rows):
        lines.append('ecoli\t%d\tGATCGA\tread%d\tt\t%d\t%.2f\t1.500\t0.00200\tGATCGA\t81.25\t1.50\t0.10'
                     % (100 + i // 2, i * 3 // n_rows, idx[i], 80.0 + (i % 7)))
        if i % 11 == 5:
            lines.append('plasmid\t5\tAAAAAA\tother\tt\t1\t70.00\t1.0\t0.001\tAAAAAA\t71.00\t1.0\t0.1')
    return '\n'.join(lines) + '\n', idx.astype(np.int32)


@pytest.mark.parametrize('n_threads', [1, 3, 7])
def test_the_host_parser_writes_the_column_with_the_indices(tmp_path, n_threads):
    """... also where the parser's threads cut the rows into pieces that begin and end inside a word of the column: a piece's
    first row is compared with the last row of the piece in front of it."""
    from mcaller_amd import _lib
    text, idx = idx_tsv(1003, 5)
    p = tmp_path / 'x.eventalign.tsv'
    p.write_text(text)
    t = _lib.parse_eventalign(str(p), 0, len(text), ['ecoli'], n_threads)
    assert t.n_rows == 1003 and np.array_equal(t.event_idx, idx) and t.n_pieces == n_threads
    assert t._idx_rel_bits is not None and len(t._idx_rel_bits) == 126
    assert np.array_equal(t.idx_rel_bits, _lib.pack_idx_rel(t.event_idx))
    assert np.array_equal(t.idx_rel_bits, rel_numpy(idx))
    planes = np.unpackbits(t.idx_rel_bits.view(np.uint8).reshape(-1, 2), axis=1, bitorder='little')
    assert planes[:, :8].sum() > 200 and planes[:, 8:].sum() > 200 and (planes[:, :8] | planes[:, 8:]).sum() < 900       # (all three relations occur)
    for s0, s1 in ((0, 1), (1, 2), (1, 3)):
        sub = t.slice_segments(s0, s1)
        assert np.array_equal(sub.idx_rel_bits, _lib.pack_idx_rel(sub.event_idx))


def test_the_synthetic_table_has_the_column():
    from mcaller_amd import synth
    codes = synth.genome(length=30000, seed=3)
    table, _ = synth.make_table(6147, seed=9, codes=codes, read_len=(300, 900))
    want = rel_numpy(table.event_idx)
    assert np.array_equal(table.idx_rel_bits, want)
    assert (want & 0x00FF).any() and (want & 0xFF00).any()      # (reads of both strands: indices that rise and that fall)
    tiled, _ = synth.tile_table(table, np.zeros(table.n_reads), 3)
    assert np.array_equal(tiled.idx_rel_bits, rel_numpy(tiled.event_idx))
    assert np.array_equal(tiled.pinned().idx_rel_bits, rel_numpy(tiled.event_idx))
