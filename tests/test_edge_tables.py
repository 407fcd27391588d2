"""The edge tables of tests/edge_tables.py, held to their claims on the CPU: a placement that misses its row tests nothing and
passes, so every claim the builder makes (this event of this read lies on this row) is checked here against the table itself
and against the records of the C oracle (oracle/mc_oracle.c).  The builder's own row-by-row walk -- it is what knows the ROWS of
a window and of a slot -- is held to the oracle as well: same records, on every table.  100 % of the claims hold; the builder
raises on a claim it cannot place.  tests/test_gpu_edges.py runs the same tables on the device."""
import collections

import numpy as np
import pytest

from tests import edge_tables as E
from tests import helpers as H

MOTIFS = ('GATC', 'A')
# claims per event kind, for one motif at one (k, skip_thresh): they follow from the lists in edge_tables.py
N_TARGETS = len(E.BIG_CUTS) * len(E.MULTIPLES) * len(E.OFFSETS) + 2 * len(E.OFFSETS) + len(E.SMALL_CUTS) * 3      # 45 + 10 + 15 = 70
N_GAP_VARIANTS = 2 + 1 + 2 + 3 * 5          # lengths 1, 2, 3: two, one, two places of the cut inside the gap; the longer ones: three
EXPECTED = {'start': N_TARGETS * 3,                                    # a read end of kind a, b and c in front of every start
            'close': N_TARGETS * 4,                                    # the closer directly behind and behind 1, 2, 3 filtered rows
            'last': N_TARGETS,                                         # (each run with tail_contig -1 and 0)
            'window': len(E.WINDOW_LENGTHS) * len(E.BIG_CUTS) * 2,     # closing row on the cut and one row behind it
            'slot': (len(E.SLOT_SIZES) + len(E.SLOT_SIZES_REPEATED)) * (len(E.BIG_CUTS) + 1),      # across each cut, and clear of them
            'gap': N_GAP_VARIANTS * len(E.BIG_CUTS),
            'f0': len(E.F0_OFFSETS) + len(E.NO_SITE_BLOCKS) + 2,       # + a palindromic first site row at offsets 0 and 1
            'violation': len(E.VIOLATION_CUTS) * 3 * 2,                # three pairs around every cut, position and event index
            'blocks': 9,                                               # 2, 3, 4 per chunk; 16, 17, 18 per staged range of either emit
            'tile': 3}                                                 # 16, 17, 18 closing rows in a tile (motif GATC over a genome with runs)
OTHER_K, OTHER_K_KINDS = E.OTHER_K, E.OTHER_K_KINDS


def test_the_geometry_is_the_kernels():
    """Whoever changes a kernel's geometry moves the edge tables with it: the numbers in edge_tables.py are the sources'."""
    for fname, name, in_source, here in E.geometry_of_the_sources():
        assert in_source is not None, '%s not found in %s: the edge tables aim at the cuts it stands for' % (name, fname)
        assert in_source == here, '%s is %d in %s and %d in tests/edge_tables.py: the edge tables must move with it' % (name, in_source, fname, here)
    assert E.PIECE == 4 * E.F_THREADS - E.FH == 960 and E.K0_ROUND == 512
    src = open(H.REPO + '/mcaller_amd/csrc/mc_fused.hip').read()
    assert 'FR = 4 * F_THREADS' in src and 'FT = FR - FH' in src
    assert E.PERIOD == np.lcm.reduce([E.PIECE, E.CHUNK, E.TILE])


def unfiltered_from(table, row):
    while row < table.n_rows and table.flags[row] & E.N_FLAG:
        row += 1
    return row


def offending_pairs(table, seg):
    """(row - 1, row, kind) of every pair of neighbouring rows of a block that a regular read does not have."""
    a, b = int(table.seg_row_begin[seg]), int(table.seg_row_begin[seg + 1])
    out = []
    if b - a < 2:
        return out
    pos, idx = table.pos[a:b].astype(np.int64), table.event_idx[a:b].astype(np.int64)
    up = idx[1] > idx[0]
    for i in np.flatnonzero(pos[1:] < pos[:-1]):
        out.append((a + int(i), a + int(i) + 1, 'pos'))
    for i in np.flatnonzero((idx[1:] <= idx[:-1]) if up else (idx[1:] >= idx[:-1])):
        out.append((a + int(i), a + int(i) + 1, 'idx'))
    return out


def records_signature(rec, k):
    n = rec.n
    return (rec.site_pos[:n].tolist(), rec.close_row[:n].tolist(), rec.info[:n].tolist(), rec.feats[:n * k].view(np.uint64).tolist())


def check_table(et, all_means=False):
    """Every claim of one edge table; -> Counter of the claims by (kind, cut)."""
    table, k, ref = et.table, et.k, et.ref
    orc = H.oracle_records(table, ref.arrays, et.qual, k, et.skip, 0.0, tail_contig=et.tail)
    w = E.walk(table, ref, k, et.skip, tail=et.tail)
    n = orc.n
    assert n == len(w.recs), '%s: the walk makes %d records, the oracle %d' % (et.name, len(w.recs), n)
    assert orc.site_pos[:n].tolist() == [r.site for r in w.recs] and orc.close_row[:n].tolist() == [r.closer for r in w.recs] and \
        orc.site_seg[:n].tolist() == [r.seg for r in w.recs], '%s: the walk and the oracle differ' % et.name
    by_closer = collections.defaultdict(list)
    for j in range(n):
        by_closer[int(orc.close_row[j])].append(j)

    def mean_is_numpys(j, dst, rows, what):
        v = E.slot_values(table, rows)
        got, want = orc.feats[j * k + dst], np.mean(v)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), '%s: %r, oracle %r, np.mean of %d values %r' % (et.name, what, got, len(v), want)

    def record_at(c, closer):
        js = [j for j in by_closer.get(closer, []) if int(orc.site_seg[j]) == c.seg]
        assert len(js) == 1, '%s: %r: %d records of the read are closed by row %d' % (et.name, c, len(js), closer)
        return js[0], w.recs[js[0]]

    if all_means:
        for j, r in enumerate(w.recs):
            if orc.info[j] & H_I_TOO_MANY():
                continue
            for dst in range(k):
                rows = r.slot_rows(dst, k)
                if rows:
                    mean_is_numpys(j, dst, rows, 'record %d slot %d' % (j, dst))
    count = collections.Counter()
    fl = table.flags
    for c in et.claims:
        count[(c.kind, c.cut)] += 1
        m = c.more
        assert 0 <= c.seg < table.n_seg and (c.row - c.offset) % c.cut == 0
        a, b = int(table.seg_row_begin[c.seg]), int(table.seg_row_begin[c.seg + 1])
        if c.kind == 'start':
            assert a == c.row and (fl[a] & E.START_FLAGS) == E.START_FLAGS, (et.name, c)
            assert m['pred_seg'] == c.seg - 1 and not (fl[a] & E.N_FLAG)
            closed = [j for j in by_closer.get(a, []) if int(orc.site_seg[j]) == c.seg - 1]
            assert bool(closed) == m['open'], (et.name, c)
            if m['pred'] == 'c':
                assert (fl[a - 2:a] & E.N_FLAG).all(), (et.name, c)
            else:
                assert not (fl[a - 1] & E.N_FLAG), (et.name, c)
                assert m['open'] if m['pred'] == 'b' else (not m['open'] or et.motif == 'A'), (et.name, c)
            if closed:
                assert w.recs[closed[0]].last_row() == unfiltered_before(table, a), (et.name, c)
        elif c.kind == 'close':
            closer = m['closer']
            assert a <= c.row < closer < b and closer == unfiltered_from(table, c.row + 1) == c.row + 1 + m['behind'], (et.name, c)
            assert not (fl[c.row] & E.N_FLAG)
            j, r = record_at(c, closer)
            assert r.last_row() == c.row and r.first_row() == m['first'], (et.name, c)
        elif c.kind == 'last':
            assert table.n_rows == c.row and b == c.row and et.tail == 0, (et.name, c)
            assert n and int(orc.close_row[n - 1]) == table.n_rows and w.recs[-1].last_row() == table.n_rows - 1, (et.name, c)
            assert w.recs[-1].first_row() == m['first']
            assert H.oracle_records(table, ref.arrays, et.qual, k, et.skip, 0.0, tail_contig=-1).n == n - 1
        elif c.kind == 'window':
            j, r = record_at(c, m['closer'])
            assert r.last_row() == c.row and r.first_row() == m['first'] == c.row - m['length'] + 1, (et.name, c)
            assert m['closer'] == c.row + 1 and a <= m['first']
        elif c.kind == 'slot':
            j, r = record_at(c, m['closer'])
            rows = r.slot_rows(m['dst'], k)
            assert rows == list(range(m['first'], m['first'] + m['size'])), (et.name, c)
            assert not (orc.info[j] & H_I_TOO_MANY())
            mean_is_numpys(j, m['dst'], rows, c)
            if m['across']:
                assert m['first'] < c.row <= m['first'] + m['size'] - 1 and c.row % c.cut == 0, (et.name, c)
            else:
                assert all(m['first'] // cut == (m['first'] + m['size']) // cut for cut in E.BIG_CUTS), (et.name, c)
        elif c.kind == 'gap':
            g0 = c.row - m['before']
            assert (fl[g0:g0 + m['length']] & E.N_FLAG).all() and not (fl[g0 - 1] & E.N_FLAG) and not (fl[g0 + m['length']] & E.N_FLAG), (et.name, c)
            assert m['closing'] == g0 - 1 and m['closer'] == g0 + m['length'] and m['closing'] < c.row <= m['closer'] and c.row % c.cut == 0
            j, r = record_at(c, m['closer'])
            assert r.last_row() == m['closing'] and a <= r.first_row() and m['closer'] < b, (et.name, c)
        elif c.kind == 'f0':
            f0 = E.first_site_of_block(table, ref, k, c.seg)
            assert b - a == m['block_rows']
            if m['block_offset'] < 0:
                assert f0 == -1 and c.row == a and w.f0[c.seg] == -1, (et.name, c)
            else:
                assert f0 == c.row == a + m['block_offset'] == w.f0[c.seg], (et.name, c, f0)
            if m['palindromic']:
                assert (fl[f0] & E.EQ_FLAG) and table.event_idx[a + 1] < table.event_idx[a], (et.name, c)
        elif c.kind == 'violation':
            bad = [(s, offending_pairs(table, s)) for s in range(table.n_seg)]
            bad = [(s, p) for s, p in bad if p]
            assert bad == [(c.seg, [(c.row - 1, c.row, m['what'])])], (et.name, c, bad)
            assert not any(offending_pairs(et.unbroken, s) for s in range(table.n_seg))
            if m['what'] == 'pos':
                whole = H.oracle_records(et.unbroken, ref.arrays, et.qual, k, et.skip, 0.0)
                assert records_signature(whole, k) != records_signature(orc, k), '%s: the violation does not show in the records' % et.name
        elif c.kind == 'tile':
            in_tile = sum(1 for r in w.recs if r.rows() and c.row <= r.last_row() < c.row + E.TILE)
            assert in_tile == m['n'] and c.row % E.TILE == 0, (et.name, c, in_tile)
        elif c.kind == 'blocks':
            sb = table.seg_row_begin
            over = int(((sb[:-1] < m['hi']) & (sb[1:] > m['lo'])).sum())
            assert over == m['n'], (et.name, c, over)
        else:
            raise AssertionError('unknown claim %r' % (c,))
    if et.kind_is_regular():
        assert not any(offending_pairs(table, s) for s in range(table.n_seg)), et.name
    return count


def H_I_TOO_MANY():
    from mcaller_amd import _lib
    return _lib.I_TOO_MANY


def unfiltered_before(table, row):
    row -= 1
    while table.flags[row] & E.N_FLAG:
        row -= 1
    return row


# (event 9 is a sparse motif's by its nature: GATC over the genome with runs of GATCGATC... in it)
@pytest.mark.parametrize('kind,motif', [(kind, motif) for kind in sorted(EXPECTED) for motif in (MOTIFS if kind != 'tile' else ('GATC' + E.RUNS,))])
def test_every_claim_holds(kind, motif, capsys):
    count = collections.Counter()
    rows = 0
    for et in E.tables(kind, motif):
        count += check_table(et, all_means=kind in ('slot', 'window'))
        rows += et.table.n_rows
    per_kind = sum(count.values())
    with capsys.disabled():
        print('\n%-9s %-4s %3d tables %7d rows %3d claims: %s' % (kind, motif, len(E.tables(kind, motif)), rows, per_kind,
                                                                 ', '.join('%d at %d' % (v, c) for (_, c), v in sorted(count.items()))))
    assert per_kind >= EXPECTED[kind], (kind, motif, per_kind, EXPECTED[kind])
    if kind in ('start', 'close', 'last'):
        per_cut = N_TARGETS and {E.PIECE: 20, E.CHUNK: 20, E.TILE: 15, E.STRIPE: 6, E.UNIT: 9}      # 3 multiples x 5 offsets (+ 5 at 15360); 2 x 3; 3 x 3
        mult = {'start': 3, 'close': 4, 'last': 1}[kind]
        for cut, want in per_cut.items():
            assert count[(kind, cut)] >= want * mult, (kind, motif, cut, count[(kind, cut)], want * mult)


@pytest.mark.parametrize('motif', MOTIFS)
@pytest.mark.parametrize('k,skip', OTHER_K)
def test_every_claim_holds_at_other_window_lengths(k, skip, motif, capsys):
    """The start, closing-row and window-length tables built again for another k / skip_thresh: which row closes a window
    depends on both."""
    for kind in OTHER_K_KINDS:
        count = collections.Counter()
        for et in E.tables(kind, motif, k, skip):
            count += check_table(et, all_means=kind == 'window')
        with capsys.disabled():
            print('\n%-9s %-4s k %d skip %d: %d claims' % (kind, motif, k, skip, sum(count.values())))
        assert sum(count.values()) >= EXPECTED[kind]
