"""The model-N bit column (mc_table_view.model_n_bits: bit r & 7 of byte r >> 3 is MC_F_MODEL_N of row r's flag byte) on the host:
the native packer against numpy, and every maker and carrier of a host table -- the parser, the synthetic table, pinned(), view(),
slice_segments() -- against the packed flag column.  No GPU."""
import ctypes as C

import numpy as np
import pytest


def packed(flags):
    return np.packbits((np.asarray(flags, dtype=np.uint8) >> 1) & 1, bitorder='little')


def small_table(seg_begin, seed, maker_column):
    """Rows with all four flag bits at random, segments at the given rows; maker_column: the table carries a bit column of its
    own (as a parser's does) instead of bare arrays."""
    from mcaller_amd import _lib
    n = int(seg_begin[-1])
    rng = np.random.default_rng(seed)
    flags = rng.integers(0, 16, size=n).astype(np.uint8)
    ns = len(seg_begin) - 1
    return _lib.Table(np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.arange(n, dtype=np.int32), flags,
                      np.asarray(seg_begin, dtype=np.int64), np.arange(ns, dtype=np.int32), np.zeros(ns, np.int32), ns,
                      model_n_bits=_lib.pack_model_n(flags) if maker_column else None)


@pytest.mark.parametrize('n_rows', [0, 1, 7, 8, 9, 63, 64, 65, 2048 + 5])
def test_pack_model_n_is_numpys_packbits(n_rows):
    from mcaller_amd import _lib
    assert _lib.F_MODEL_N == 2
    rng = np.random.default_rng(1000 + n_rows)
    flags = rng.integers(0, 16, size=n_rows).astype(np.uint8)
    n_bytes = (n_rows + 7) // 8
    out = np.full(n_bytes + 8, 0xA5, dtype=np.uint8)        # (every byte of the column is written, none behind it)
    _lib.lib().mc_pack_model_n(flags.ctypes.data_as(C.c_void_p), n_rows, out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out[:n_bytes], packed(flags)) and (out[n_bytes:] == 0xA5).all()
    assert np.array_equal(_lib.pack_model_n(flags), packed(flags))


@pytest.mark.parametrize('maker_column', [False, True])
def test_slice_segments_at_every_offset_inside_a_byte(maker_column):
    """Segments that start at rows with r0 % 8 of 0, 1 and 7 (and end inside a byte): the slice's column is its flags, packed."""
    seg_begin = [0, 16, 33, 47, 64, 81, 103, 128, 131]
    t = small_table(seg_begin, 7, maker_column)
    assert np.array_equal(t.model_n_bits, packed(t.flags))
    seen = set()
    for s0 in range(len(seg_begin) - 1):
        for s1 in range(s0 + 1, len(seg_begin)):
            sub = t.slice_segments(s0, s1)
            assert np.array_equal(sub.flags, t.flags[seg_begin[s0]:seg_begin[s1]])
            assert np.array_equal(sub.model_n_bits, packed(sub.flags)), (s0, s1)
            seen.add(seg_begin[s0] % 8)
    assert {0, 1, 7} <= seen


@pytest.mark.parametrize('maker_column', [False, True])
def test_pinned_and_view_carry_the_column(maker_column):
    from mcaller_amd import _lib
    t = small_table([0, 10, 21], 11, maker_column)
    want = packed(t.flags)
    p = t.pinned()
    assert p._model_n_bits is not None and np.array_equal(p.model_n_bits, want)
    assert _lib.lib().mc_host_is_pinned is not None and p.model_n_bits.ctypes.data != t.model_n_bits.ctypes.data
    for tab in (t, p):
        v = tab.view()
        assert v.model_n_bits and v.flags
        got = np.frombuffer((C.c_char * len(want)).from_address(v.model_n_bits), dtype=np.uint8)
        assert np.array_equal(got, want)
    assert p.view().model_n_bits == p.model_n_bits.ctypes.data      # (the pinned block itself: nothing is packed per upload)


def test_bare_arrays_are_packed_from_the_flags_as_they_are():
    """A table made from bare arrays whose flags are edited afterwards (the tests' gap tables do) hands out the edited column."""
    from mcaller_amd import _lib
    t = small_table([0, 40], 13, False)
    t.flags[:] = 0
    t.flags[9] = _lib.F_MODEL_N
    assert np.array_equal(t.model_n_bits, packed(t.flags)) and t.model_n_bits[1] == 2


def n_tsv(n_rows, seed):
    """eventalign lines of two reads on one contig, a third of them with an NNNNNN model k-mer; a header and lines of an unknown
    contig between them."""
    rng = np.random.default_rng(seed)
    lines = ['contig\tposition\treference_kmer\tread_name\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\tmodel_kmer\tmodel_mean\tmodel_stdv\tstandardized_level']
    is_n = []
    for i in range(n_rows):
        n = bool(rng.random() < 0.35)
        is_n.append(n)
        lines.append('ecoli\t%d\tGATCGA\tread%d\tt\t%d\t%.2f\t1.500\t0.00200\t%s\t%.2f\t1.50\t0.10'
                     % (100 + i // 2, i * 3 // n_rows, i, 80.0 + (i % 7), 'NNNNNN' if n else 'GATCGA', 0.0 if n else 81.25))
        if i % 11 == 5:
            lines.append('plasmid\t5\tAAAAAA\tother\tt\t1\t70.00\t1.0\t0.001\tAAAAAA\t71.00\t1.0\t0.1')
    return '\n'.join(lines) + '\n', np.array(is_n)


@pytest.mark.parametrize('n_threads', [1, 3, 7])
def test_the_host_parser_writes_the_column_with_the_flags(tmp_path, n_threads):
    """... also where the parser's threads cut the rows into pieces that end inside a byte of the column."""
    from mcaller_amd import _lib
    text, is_n = n_tsv(1003, 5)
    p = tmp_path / 'n.eventalign.tsv'
    p.write_text(text)
    t = _lib.parse_eventalign(str(p), 0, len(text), ['ecoli'], n_threads)
    assert t.n_rows == 1003 and np.array_equal((t.flags & _lib.F_MODEL_N) != 0, is_n)
    assert t._model_n_bits is not None and len(t._model_n_bits) == 126
    assert np.array_equal(t.model_n_bits, packed(t.flags))
    assert np.array_equal(t.slice_segments(1, 2).model_n_bits, packed(t.slice_segments(1, 2).flags))


def test_the_synthetic_table_has_the_column():
    from mcaller_amd import synth
    codes = synth.genome(length=30000, seed=3)
    table, _ = synth.make_table(6147, seed=9, codes=codes, read_len=(300, 900))
    assert int((table.flags & 2 != 0).sum()) > 50
    assert np.array_equal(table.model_n_bits, packed(table.flags))
    tiled, _ = synth.tile_table(table, np.zeros(table.n_reads), 3)
    assert np.array_equal(tiled.model_n_bits, packed(tiled.flags))
    assert np.array_equal(tiled.pinned().model_n_bits, packed(tiled.flags))
