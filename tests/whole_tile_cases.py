"""Tables for k1_scan's whole-tile path (the instances that stream unit summaries take a tile that lies inside ONE name block in a
single batch: scan_tile_is_whole, mc_dev.h).  TEST INFRASTRUCTURE: tests/test_whole_tile_cases.py holds what is claimed here on the
CPU, tests/test_gpu_scan_whole_tile.py runs the tables through the passes and asks the library which tiles took the path.

Every table has three tiles of 2048 rows plus 1, 3 or 7 rows; the tile under test is tile 1 (rows 2048 .. 4095) unless said
otherwise.  A case: (name, table, read qualities, quality threshold, expected whole-tile flags per tile, more) -- `more` holds what
the construction claims beyond that (rows that are the last row of a window, the units a tile lists, an unbroken twin).
Reads come from a seeded pool of reads of 9000 positions and more (tests/edge_tables.py's Pool and Read), cut and laid one behind
the other."""
import functools

import numpy as np

from mcaller_amd import synth
from tests import edge_tables as E

TILE, CHUNK, STRIPE, UNIT, CG = E.TILE, E.CHUNK, E.STRIPE, E.UNIT, 64
T0 = TILE                           # first row of the tile under test
SIZES = (6145, 6147, 6151)
MOTIFS = ('GATC', 'GTAC')           # both sparse: one position in 256 per strand
K, SKIP = 6, 0
LOW_QUAL, QUAL_THRESH = 5.0, 7.0    # (the pool's qualities lie in 6 .. 12: a case that filters gives every other read 8 or more)


class Case(object):
    def __init__(self, name, table, qual, whole, qual_thresh=0.0, repeated=False, **more):
        self.name, self.table, self.qual, self.whole, self.qual_thresh, self.repeated, self.more = name, table, qual, list(whole), qual_thresh, repeated, more

    def __repr__(self):
        return '%s [%d rows]' % (self.name, self.table.n_rows)


@functools.lru_cache(maxsize=None)
def long_pool():
    p = E.Pool(8104, (9000, 9600), 330000)
    assert len(p.reads) >= 12 and min(len(r) for r in p.reads) >= 8300
    return p


def reads_of(up=None, start=0):
    """The pool's reads from `start` on, round and round; up: only those whose event indices rise (True) or fall (False)."""
    reads = long_pool().reads
    for i in range(start, start + 4 * len(reads)):
        r = reads[i % len(reads)]
        if up is None or r.up() == up:
            yield r


def filler(n, start):
    """n rows of a read of their own (the first row not filtered)."""
    for r in reads_of(start=start):
        for a in range(0, 200):
            if not r.fl[a] & E.N_FLAG:
                return r.cut(a, a + n)
    raise AssertionError('no filler')


def lay(blocks, n_rows, start=3):
    """The blocks one behind the other, a filler behind them up to n_rows rows -> (table, qualities)."""
    n = sum(len(b) for b in blocks)
    assert n < n_rows, (n, n_rows)
    blocks = list(blocks) + [filler(n_rows - n, start)]
    t, q = E.table_of(blocks)
    return t, np.maximum(q, 8.0)


def site_rows(r, ref):
    offs = ref.site_off(K)[0 if r.up() else 1]
    return [i for i in range(len(r)) if not (r.fl[i] & E.N_FLAG) and offs[int(r.pos[i])] >= 0]


def block_with_first_site_at(ref, d, n, start, palindromic=False):
    """A block of n rows whose first site row is its row d.  palindromic: a read whose indices fall and whose first site row has
    the reference's k-mer as its model k-mer (R5: the row opens a one-event '+' window, the block is tested from row d + 1 on)."""
    offs = ref.site_off(K)
    for r in reads_of(up=not palindromic, start=start):
        if palindromic:
            zs = [i for i in range(len(r)) if (r.fl[i] & E.EQ_FLAG) and not (r.fl[i] & E.N_FLAG) and offs[0][int(r.pos[i])] >= 0]
        else:
            zs = site_rows(r, ref)
        for z in zs:
            if z < d or z - d + n > len(r) or (r.fl[z - d] & E.N_FLAG):
                continue
            probe = r.cut(z - d, z - d + n)
            if E.alone(probe, ref, K, SKIP).f0[0] == d and E.first_site_of_block(E.table_of([probe])[0], ref, K, 0) == d:
                return probe
    raise AssertionError('no block of %d rows with its first site row at %d' % (n, d))


def eligibility_cases(motif, n_rows):
    """Tile 1 next to every edge of the predicate."""
    ref = E.ref_of(motif)
    out = []

    def one(name, a, d, n, whole, pal=False):
        b = block_with_first_site_at(ref, d, n, len(out), pal)
        t, q = lay([filler(a, 5 + len(out)), b], n_rows)
        assert int(t.seg_row_begin[1]) == a and int(t.seg_row_begin[2]) == a + n
        assert E.walk(t, ref, K, SKIP).f0[1] == a + d
        out.append(Case('%s, %s' % (motif, name), t, q, whole, block=(a, a + n), f0=a + d))

    on, off = [False, True, False, False], [False] * 4
    one('the block begins at t0 - 1, is tested from t0 on and ends at t0 + TILE', T0 - 1, 1, TILE + 1, on)
    one('the block begins at t0', T0, 0, TILE + 200, off)
    one('the block begins at t0 + 1', T0 + 1, 0, TILE + 200, off)
    one('the block ends at t0 + TILE - 1', T0 - 1, 1, TILE, off)
    one('the block is tested from t0 + 1 on', T0 - 1, 2, TILE + 1, off)
    one('the block begins eight rows in front of t0 and ends eight rows behind the tile', T0 - 8, 3, TILE + 16, on)
    one('a palindromic first site row at t0 - 1, the block\'s first: the extra row in front of the tile', T0 - 1, 0, TILE + 100, on, pal=True)
    # two path tiles side by side, the second one under the same block; the last, partial tile is never on the path
    b = block_with_first_site_at(ref, 4, n_rows - 1001, 3)
    t, q = lay([filler(1000, 9), b], n_rows)
    out.append(Case('%s, one block from row 1000 to the last row but one' % motif, t, q, [False, True, True, False]))
    # a block that is filtered by its read's quality
    b = block_with_first_site_at(ref, 4, 3000, 5)
    t, q = lay([filler(2000, 11), b], n_rows)
    q[1] = LOW_QUAL
    out.append(Case('%s, the tile under a block that is filtered by quality' % motif, t, q, on, qual_thresh=QUAL_THRESH))
    # a block without a site row: a stretch of a read that covers no marked position, every row of it many times
    for r in reads_of(up=True, start=2):
        s = site_rows(r, ref)
        gaps = [(z - a - 1, a + 1) for a, z in zip([-1] + s, s + [len(r)])]
        g, a = max(gaps)
        if g < 100:
            continue
        while r.fl[a] & E.N_FLAG:
            a, g = a + 1, g - 1
        quiet = r.cut(a, a + g)
        quiet = quiet.repeated(np.full(len(quiet), 2400 // len(quiet) + 1)).cut(0, 2400)
        assert E.alone(quiet, ref, K, SKIP).f0[0] == -1
        break
    t, q = lay([filler(2000, 12), quiet], n_rows)
    out.append(Case('%s, the tile under a block without a site row' % motif, t, q, on))
    return out


def block_with_a_window_ending_at(ref, row, j, n, start, up=True):
    """A block of n rows in which row `row` is the last contributing row of a window and j filtered rows lie between it and the
    row that closes the window."""
    for r in reads_of(up=up, start=start):
        for rec in E.alone(r, ref, K, SKIP).recs:
            z = rec.last_row()
            if z < row or rec.closer != z + 1 or rec.closer >= len(r) or z - row + n > len(r) or (r.fl[z - row] & E.N_FLAG):
                continue
            probe = r.cut(z - row, len(r)).with_filtered_behind(row, j).cut(0, n)
            w = E.alone(probe, ref, K, SKIP)
            if any(x.last_row() == row and x.closer == row + 1 + j for x in w.recs):
                return probe
    raise AssertionError('no block with a window whose last row is row %d' % row)


# tile rows on the former chunk edge, the stripe edges and the tile's last rows, and how many filtered rows lie behind each
EDGE_ROWS = [(1021, 0), (1022, 1), (1023, 2), (1024, 0), (1025, 1), (1026, 2), (1022, 2), (1023, 0), (1023, 1), (1024, 2),
             (511, 0), (511, 1), (511, 2), (510, 2), (512, 0), (1535, 1), (1535, 2), (1536, 0), (2046, 0), (2046, 1), (2046, 2),
             (2047, 0), (2047, 1), (2047, 2)]


def chunk_edge_cases(motif, n_rows):
    """A window's last row on the former chunk edge, the stripe edges and the tile's last rows, closed by the next row, the row
    behind one filtered row, the row behind two (out of line).  The block begins at row 0: tiles 1 and 2 are on the path."""
    ref = E.ref_of(motif)
    out = []
    for ci, (row, j) in enumerate(EDGE_ROWS):
        b = block_with_a_window_ending_at(ref, T0 + row, j, n_rows - 1, ci, up=ci % 3 != 2)
        t, q = lay([b], n_rows)
        w = E.walk(t, ref, K, SKIP)
        assert any(x.last_row() == T0 + row and x.closer == T0 + row + 1 + j for x in w.recs)
        out.append(Case('%s, a window whose last row is tile row %d, %d filtered rows behind it' % (motif, row, j), t, q,
                        [False, True, True, False], last_row=T0 + row, closer=T0 + row + 1 + j))
    return out


# the second row of the violating pair, as a row of tile 1: a unit edge, a stripe edge, row 1024, the tile's last row
VIOLATION_ROWS = (8, 512, 1024, 2047)
VIOLATION_KINDS = ('pdec', 'pos0', 'eq', 'inc', 'dec')


def violation_cases(motif, n_rows):
    """One violating pair inside a path tile; every case carries its unbroken twin (more['unbroken']: the same rows without the
    violation, whose tiles are on the path as a REGULAR block's)."""
    ref = E.ref_of(motif)
    out = []
    for vi, row in enumerate(VIOLATION_ROWS):
        for ki, kind in enumerate(VIOLATION_KINDS):
            up = kind != 'inc'                          # ('inc': an increase in a block whose indices fall)
            target = T0 + row
            for b in reads_of(up=up, start=vi * 5 + ki):
                b = b.cut(0, n_rows - 1)
                if b.fl[0] & E.N_FLAG or not E.alone(b, ref, K, SKIP).recs or int(b.pos[target - 1]) < 2:
                    continue
                break
            good = b
            bad = b.cut(0, len(b))
            if kind == 'pdec':
                bad.pos[target] = bad.pos[target - 1] - 1
            elif kind == 'pos0':
                bad.pos[target] = 0
            elif kind == 'eq':
                bad.idx[target:] += -1 if up else 1
            else:
                bad.idx[target:] += -2 if up else 2
            d = np.sign(np.diff(bad.idx.astype(np.int64)))
            sign = 1 if up else -1
            assert d[target - 1] == {'eq': 0, 'inc': 1, 'dec': -1}.get(kind, sign) and (np.delete(d, target - 1) == sign).all()
            dp = np.diff(bad.pos.astype(np.int64))
            assert (dp[target - 1] < 0) == (kind in ('pdec', 'pos0')) and (np.delete(dp, [target - 1, target]) >= 0).all()
            t, q = lay([bad], n_rows)
            t_good, _ = lay([good], n_rows)
            out.append(Case('%s, %s at tile rows (%d, %d)' % (motif, kind, row - 1, row), t, q, [False, True, True, False], repeated=True,
                            unbroken=t_good, pair=(target - 1, target)))
    return out


# ---- a tile that lists more than CG units, but no more than CG in either chunk ----
def listed_units(table, marked, rev, t0):
    """The units of the tile at t0 that the scan's filter lists when the tile lies in one regular block of strand `rev`: the mask
    bits [p0, p7 + k) hold a marked position, or they are more than 32 (the filter of k1_scan, restated)."""
    out = []
    for u in range(TILE // UNIT):
        p0, p7 = int(table.pos[t0 + u * UNIT]), int(table.pos[t0 + u * UNIT + UNIT - 1])
        span = p7 - p0 + K
        if not 0 < span <= 32 or marked[rev][p0:p0 + span].any():
            out.append(u)
    return out


@functools.lru_cache(maxsize=None)
def rich_case(motif, n_rows):
    """A reference that is the pool's genome with ONE stretch of the motif repeated end to end in it -- sparse overall -- and a
    read through the stretch laid so that the stretch straddles tile 1's chunk edge."""
    base = E.genome_of('')
    code = {'A': 0, 'C': 1, 'G': 2, 'T': 3}
    for r in reads_of(up=True, start=4):
        if len(r) < n_rows:
            continue
        for length in range(300, 900, 12):
            for shift in (0, 40, -40, 80, -80):
                mid = T0 + CHUNK + shift
                lo = int(r.pos[mid]) - length // 2
                codes = base.copy()
                codes[lo:lo + length] = np.tile(np.array([code[c] for c in motif], dtype=np.uint8), length // len(motif) + 1)[:length]
                sref = synth.SynthRef(codes, motif=motif)
                marked = [np.frombuffer(m.encode('latin1'), dtype=np.uint8) == ord('M') for m in sref.meth[0]]
                b = r.cut(0, n_rows - 1)
                if b.fl[0] & E.N_FLAG:
                    continue
                t, q = lay([b], n_rows)
                units = listed_units(t, marked, 0, T0)
                first, second = [u for u in units if u < CHUNK // UNIT], [u for u in units if u >= CHUNK // UNIT]
                if CG < len(units) <= 2 * CG and len(first) <= CG and len(second) <= CG and len(first) > 20 and len(second) > 20:
                    n_sites = int(marked[0].sum() + marked[1].sum())
                    assert n_sites * 64 <= len(codes), 'the reference is not sparse: %d sites in %d bases' % (n_sites, len(codes))
                    return Case('%s, a tile that lists %d + %d units' % (motif, len(first), len(second)), t, q, [False, True, True, False],
                                arrays=sref.device_arrays(), units=(len(first), len(second)), n_sites=n_sites, genome=len(codes))
    raise AssertionError('no stretch found')


def slot_reuse_tables(motif):
    """(longer table: tile 1 on the path, shorter table: a block edge inside tile 1)."""
    ref = E.ref_of(motif)
    b = block_with_first_site_at(ref, 4, 5000, 6)
    longer = lay([filler(1000, 13), b], 6151)
    b1, b2 = block_with_first_site_at(ref, 2, 2000, 7), block_with_first_site_at(ref, 3, 2100, 8)
    shorter = lay([filler(1000, 14), b1, b2], 6145)
    return (Case('%s, the longer table' % motif, longer[0], longer[1], [False, True, False, False]),
            Case('%s, the shorter table, a block edge at row 3000' % motif, shorter[0], shorter[1], [False] * 4))


def size_of(motif, group):
    return SIZES[(MOTIFS.index(motif) + group) % 3]
