"""What tests/whole_tile_cases.py claims of its tables, held on the CPU: which tiles satisfy the scan's whole-tile predicate
(scan_tile_is_whole, mc_dev.h: restated here from the blocks' edges and first site rows), that the C oracle finds records in
them, and that the site-rich tile lists what it is said to list."""
import numpy as np
import pytest

from tests import edge_tables as E
from tests import helpers as H
from tests import whole_tile_cases as W


def whole_tiles(case, ref):
    """The predicate per tile: the tile is full and lies inside one block, behind the block's first row, and the block is not
    regular (filtered, no site row; a violation makes it irregular) or is tested from the tile's first row on at the latest."""
    t = case.table
    f0 = E.walk(t, ref, W.K, W.SKIP).f0
    sb = [int(x) for x in t.seg_row_begin]
    out = []
    for t0 in range(0, t.n_rows, W.TILE):
        seg = int(np.searchsorted(sb, t0, side='right')) - 1
        a, b = sb[seg], sb[seg + 1]
        ok = t0 + W.TILE <= t.n_rows and a < t0 and b >= t0 + W.TILE
        if ok and not case.repeated and case.qual[seg] >= case.qual_thresh and f0[seg] >= 0:
            falls = t.event_idx[a + 1] < t.event_idx[a]
            first = f0[seg] + (1 if falls and (t.flags[f0[seg]] & E.EQ_FLAG) else 0)        # (R5: the row behind the extra row)
            ok = first <= t0
        out.append(bool(ok))
    return out


def all_cases(motif):
    out = []
    for gi, make in enumerate((W.eligibility_cases, W.chunk_edge_cases, W.violation_cases)):
        out += make(motif, W.size_of(motif, gi))
    out += list(W.slot_reuse_tables(motif))
    return out


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_the_tiles_are_on_the_path_they_are_said_to_be(motif):
    ref = E.ref_of(motif)
    cases = all_cases(motif)
    assert len(cases) >= 10 + len(W.EDGE_ROWS) + len(W.VIOLATION_ROWS) * len(W.VIOLATION_KINDS) + 2
    n_on = 0
    for c in cases:
        assert c.table.n_rows in W.SIZES and len(c.whole) == 4 and not c.whole[3] and not c.whole[0]
        assert whole_tiles(c, ref) == c.whole, c
        n_on += sum(c.whole)
        if 'unbroken' in c.more:
            twin = W.Case(c.name, c.more['unbroken'], c.qual, c.whole)
            assert whole_tiles(twin, ref) == c.whole, c
        orc = H.oracle_records(c.table, ref.arrays, c.qual, W.K, W.SKIP, c.qual_thresh)
        assert orc.n > 0, c
        if 'closer' in c.more:
            assert c.more['closer'] in [int(x) for x in orc.close_row[:orc.n]], c
    assert n_on > len(cases)


@pytest.mark.parametrize('motif', W.MOTIFS)
def test_the_site_rich_tile(motif):
    c = W.rich_case(motif, W.size_of(motif, 3))
    a, b = c.more['units']
    assert W.CG < a + b <= 2 * W.CG and a <= W.CG and b <= W.CG
    assert c.more['n_sites'] * 64 <= c.more['genome']
    orc = H.oracle_records(c.table, c.more['arrays'], c.qual, W.K, W.SKIP, 0.0)
    in_tile = (np.asarray(orc.close_row[:orc.n]) >= W.T0) & (np.asarray(orc.close_row[:orc.n]) < W.T0 + W.TILE)
    assert int(in_tile.sum()) > 40, c          # (a stretch of 300 bases and more of a four-base motif: 75 sites and more)
