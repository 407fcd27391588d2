"""The two columns a table's maker writes with the positions (DevTable::unit_pp, DevTable::prel), as numpy says them: the
reference tests/test_gpu_unit_columns.py holds the device's columns against, checked here against cases written out by hand.

unit summaries   [ceil(n / 8), 2] int32: pos[8u] and pos[8u + 7]; the second of a last, partial unit is unspecified
position relations   [ceil(n / 8)] uint16, row r = 8u + e: bit e of word u is pos[r] < pos[r - 1] (the row before it in the
                 table; row 0: clear), bit 8 + e is pos[r] == 0; the bits of rows beyond the last are 0"""
import numpy as np
import pytest

SIZES = (0, 1, 7, 8, 9, 6145, 6147, 6151)


def pos_rel_bits(pos):
    pos = np.asarray(pos, dtype=np.int32)
    n = len(pos)
    dec = np.zeros((n + 7) // 8 * 8, dtype=np.uint8)
    zero = np.zeros_like(dec)
    if n > 1:
        dec[1:n] = np.diff(pos.astype(np.int64)) < 0
    zero[:n] = pos == 0
    lo = np.packbits(dec.reshape(-1, 8), axis=1, bitorder='little')[:, 0].astype(np.uint16)
    hi = np.packbits(zero.reshape(-1, 8), axis=1, bitorder='little')[:, 0].astype(np.uint16)
    return lo | (hi << 8)


def unit_summaries(pos):
    """(first [ceil(n / 8)], last [n // 8]): the last position of whole units only."""
    pos = np.asarray(pos, dtype=np.int32)
    return pos[0::8].copy(), pos[7::8].copy()


def test_by_hand_small():
    assert pos_rel_bits([]).tolist() == [] and [a.tolist() for a in unit_summaries([])] == [[], []]
    assert pos_rel_bits([5]).tolist() == [0x0000]
    assert pos_rel_bits([0]).tolist() == [0x0100]
    # row:            0  1  2  3  4  5  6
    seven = [3, 3, 2, 0, 0, 7, 6]
    assert pos_rel_bits(seven).tolist() == [0b0001100001001100]       # less: rows 2, 3, 6; zero: rows 3, 4
    assert [a.tolist() for a in unit_summaries(seven)] == [[3], []]
    eight = seven + [5]
    assert pos_rel_bits(eight).tolist() == [0b0001100011001100]
    assert [a.tolist() for a in unit_summaries(eight)] == [[3], [5]]
    # the ninth row against the eighth: bit 0 of the second word
    assert pos_rel_bits(eight + [4]).tolist() == [0b0001100011001100, 0x0001]
    assert pos_rel_bits(eight + [5]).tolist() == [0b0001100011001100, 0x0000]
    assert pos_rel_bits(eight + [0]).tolist() == [0b0001100011001100, 0x0101]
    assert [a.tolist() for a in unit_summaries(eight + [4])] == [[3, 4], [5]]
    # the extremes of int32 do not wrap
    assert pos_rel_bits([2**31 - 1, -2**31, 2**31 - 1]).tolist() == [0x0002]


@pytest.mark.parametrize('n', SIZES)
def test_sizes(n):
    rng = np.random.RandomState(n)
    pos = rng.randint(0, 4, size=n).astype(np.int32)        # (many equal neighbours, many zeros)
    rel = pos_rel_bits(pos)
    first, last = unit_summaries(pos)
    assert rel.dtype == np.uint16 and len(rel) == (n + 7) // 8 == len(first) and len(last) == n // 8
    for r in range(n):                                      # the definition, row by row
        w = int(rel[r >> 3])
        assert (w >> (r & 7)) & 1 == (1 if r > 0 and pos[r] < pos[r - 1] else 0)
        assert (w >> (8 + (r & 7))) & 1 == (1 if pos[r] == 0 else 0)
    if n % 8:                                               # nothing beyond the last row
        assert int(rel[-1]) & ~(((1 << (n % 8)) - 1) * 0x0101) == 0
    assert all(first[u] == pos[8 * u] for u in range(len(first))) and all(last[u] == pos[8 * u + 7] for u in range(len(last)))
    # a rising table has no bit at all but row 0's "is 0"
    up = np.arange(n, dtype=np.int32)
    assert pos_rel_bits(up).sum() == (0x0100 if n else 0)
    # a falling one has every "less" bit but row 0's
    down = (n + 5 - np.arange(n)).astype(np.int32)
    want = np.full((n + 7) // 8, 0x00FF, dtype=np.uint16)
    if n:
        want[0] = 0x00FE
        if n % 8:
            want[-1] &= (1 << (n % 8)) - 1
    assert np.array_equal(pos_rel_bits(down), want)
