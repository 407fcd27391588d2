"""Edge tables: seeded eventalign tables in which a named EVENT of a probe read lies on a named table ROW -- the rows at which the
kernels of the hot path cut a table (units of 8 rows, stripes and rounds of 512, pieces of 960, chunks of 1024, tiles of 2048).
TEST INFRASTRUCTURE: tests/test_edge_tables.py holds every claim made here against the C oracle on the CPU,
tests/test_gpu_edges.py runs the tables through every way the library scans a table.

The mechanism: reads of a seeded pool (synth.make_table: rows, flags and event indices as it makes them) are cut to the number
of rows that is needed (a read cut short at its end is still a regular read; a pad of 1-7 rows is a block shorter than a unit)
and laid one behind the other; a PROBE read is changed in place (rows repeated, rows filtered, its head cut off), analysed ALONE by
walk() -- a row-at-a-time restatement of the window machine in Python that keeps the ROWS of every slot -- and put so far behind the
pads that its event lands on the target row.  A target that lies behind the current row already moves on by PERIOD =
lcm(960, 1024, 2048) rows: every residue stays what it was.  A claim that cannot be placed raises.

Words: a window's CLOSING ROW is its last contributing row (the last unfiltered row in front of the closer); its CLOSER is the
next unfiltered row, the one at which the machine flushes -- the `close_row` of the record."""
import functools
import heapq
import re
import os

import numpy as np

from mcaller_amd import _lib, synth

# ---- the geometry of the kernels, written once (tests/test_edge_tables.py reads it back from the sources) ----
UNIT = 8              # rows per unit of k1_scan
STRIPE = 512          # rows per stripe of k1_scan
K0_FS = 8             # MC_K0_FS: stripes of 64 rows per round of k0_first_site
K0_ROUND = 64 * K0_FS
TILE = 2048           # MC_TILE
CHUNK = 1024          # MC_CHUNK
ET = 1024             # MC_ET: rows per piece of k1_emit_runs
EH = 128              # MC_EH: ... and in front of it
E_MAXB = 16
FH = 64               # MC_FH: rows in front of a piece of k1_fused
F_THREADS = 256
PIECE = 4 * F_THREADS - FH      # FT = 960
F_MAXB = 16           # MC_F_MAXB
WROWS = 64
FRONT = 64
PT = 16
BIG_CUTS = (PIECE, CHUNK, TILE)
MULTIPLES = (1, 2, 5)
OFFSETS = (-2, -1, 0, 1, 2)
COINCIDE = 15360      # = 16 * 960 = 15 * 1024
SMALL_CUTS = (8, 40, 104, 512, 1536)       # 8 j for a few j, and 512; offsets -1, 0, +1
PERIOD = 30720        # lcm(960, 1024, 2048)
OTHER_K = ((4, 0), (8, 0), (6, 1))       # (k, skip_thresh) besides (6, 0), for the start / closing-row / window-length tables
OTHER_K_KINDS = ('start', 'close', 'window')
assert PERIOD % PIECE == 0 and PERIOD % CHUNK == 0 and PERIOD % TILE == 0 and COINCIDE % PIECE == 0 and COINCIDE % CHUNK == 0

GEOMETRY_IN_SOURCES = [      # (file under mcaller_amd/csrc, name, value here)
    ('mc_dev.h', 'MC_TILE', TILE), ('mc_dev.h', 'MC_CHUNK', CHUNK), ('mc_dev.h', 'WROWS', WROWS), ('mc_dev.h', 'FRONT', FRONT),
    ('mc_dev.h', 'PT', PT), ('mc_fused.hip', 'MC_FH', FH), ('mc_fused.hip', 'F_THREADS', F_THREADS), ('mc_fused.hip', 'MC_F_MAXB', F_MAXB),
    ('mc_emit.hip', 'MC_ET', ET), ('mc_emit.hip', 'MC_EH', EH), ('mc_emit.hip', 'E_MAXB', E_MAXB), ('mc_k0.hip', 'MC_K0_FS', K0_FS)]


def geometry_of_the_sources():
    """[(file, name, value in the source or None, value here)]: `#define NAME n` or `constexpr int NAME = n;`."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mcaller_amd', 'csrc')
    out = []
    for fname, name, here in GEOMETRY_IN_SOURCES:
        text = open(os.path.join(src, fname)).read()
        m = re.search(r'^\s*(?:#\s*define\s+%s\s+|constexpr\s+int\s+%s\s*=\s*)(\d+)\b' % (name, name), text, re.M)
        out.append((fname, name, int(m.group(1)) if m else None, here))
    return out


N_FLAG, EQ_FLAG = _lib.F_MODEL_N, _lib.F_KMER_EQ
START_FLAGS = _lib.F_SEG_START | _lib.F_NAME_START
GENOME_LEN, GENOME_SEED = 150000, 4711
RUNS = '+runs'        # 'GATC+runs': the motif GATC over the genome with short runs of GATCGATC... in it (event 9)
RUN_EVERY, RUN_REPEATS = 7500, 22


def genome_of(motif):
    codes = synth.genome(length=GENOME_LEN, seed=GENOME_SEED)
    if motif.endswith(RUNS):
        for at in range(RUN_EVERY, GENOME_LEN - RUN_EVERY, RUN_EVERY):
            codes[at:at + 4 * RUN_REPEATS] = np.tile(np.array([2, 0, 3, 1], dtype=np.uint8), RUN_REPEATS)
    return codes


# ---------------------------------------------------------------------------------------------------
# the reference, the reads
# ---------------------------------------------------------------------------------------------------
class Ref(object):
    def __init__(self, motif):
        self.motif = motif
        self.codes = genome_of(motif)
        self.ref = synth.SynthRef(self.codes, motif=motif[:-len(RUNS)] if motif.endswith(RUNS) else motif)
        self.arrays = self.ref.device_arrays()
        self.marked = [np.frombuffer(m.encode('latin1'), dtype=np.uint8) == ord('M') for m in self.ref.meth[0]]
        self._off = {}

    def site_off(self, k):
        """([fwd], [rev]) lists: offset of the first marked position in [p, p + k) for every p, -1 if none."""
        if k not in self._off:
            res = []
            for m in self.marked:
                mm = np.concatenate([m, np.zeros(k, dtype=bool)])
                off = np.full(len(m), -1, dtype=np.int64)
                for i in range(k - 1, -1, -1):
                    off[mm[i:i + len(m)]] = i
                res.append(off.tolist())
            self._off[k] = res
        return self._off[k]


@functools.lru_cache(maxsize=None)
def ref_of(motif):
    return Ref(motif)


class Read(object):
    """The rows of one read (one segment, one name block)."""

    def __init__(self, pos, ev, mu, idx, fl, qual):
        self.pos, self.ev, self.mu, self.idx, self.fl, self.qual = pos, ev, mu, idx, fl, qual

    def __len__(self):
        return len(self.pos)

    def up(self):
        return len(self) < 2 or self.idx[1] > self.idx[0]

    def cut(self, a, b):
        """Rows [a, b) as a read of their own: the start flags on its new first row."""
        fl = self.fl[a:b].copy()
        fl[0] |= START_FLAGS
        return Read(self.pos[a:b].copy(), self.ev[a:b].copy(), self.mu[a:b].copy(), self.idx[a:b].copy(), fl, self.qual)

    def repeated(self, count):
        """Row i `count[i]` times in place (with_stalls of test_gpu_parity.py, the counts GIVEN), event indices renumbered."""
        count = np.asarray(count, dtype=np.int64)
        fl = np.repeat(self.fl, count)
        first = np.concatenate([[True], np.diff(np.repeat(np.arange(len(self)), count)) != 0])
        fl[~first] &= np.uint8(0xFF ^ START_FLAGS)
        n = len(fl)
        idx = self.idx[0] + (np.arange(n) if self.up() else -np.arange(n))
        if idx.min() < 0:
            idx = idx - idx.min()
        return Read(np.repeat(self.pos, count), np.repeat(self.ev, count), np.repeat(self.mu, count), idx.astype(np.int32), fl, self.qual)

    def stalled(self, row, n):
        count = np.ones(len(self), dtype=np.int64)
        count[row] = n
        return self.repeated(count)

    def filtered(self, a, b):
        """Rows [a, b) turned into rows of the model k-mer NNNNNN (with_model_gaps of test_gpu_fused.py)."""
        r = self.cut(0, len(self))
        r.fl[a:b] |= N_FLAG
        r.fl[a:b] &= np.uint8(0xFF ^ EQ_FLAG)
        return r

    def with_filtered_behind(self, row, j):
        """j filtered rows put in behind `row` (copies of it)."""
        if j == 0:
            return self
        r = self.stalled(row, j + 1)
        return r.filtered(row + 1, row + 1 + j)


class Pool(object):
    def __init__(self, seed, read_len, n_rows, genome=''):
        table, qual = synth.make_table(n_rows, seed=seed, codes=genome_of(genome), read_len=read_len)
        sb = table.seg_row_begin
        self.reads = [Read(table.pos[sb[s]:sb[s + 1]], table.event_e4[sb[s]:sb[s + 1]], table.model_e4[sb[s]:sb[s + 1]],
                           table.event_idx[sb[s]:sb[s + 1]], table.flags[sb[s]:sb[s + 1]], float(qual[s])) for s in range(table.n_seg - 1)]
        self.reads = [r for r in self.reads if len(r) >= 40 and int(r.pos[0]) > 8]


@functools.lru_cache(maxsize=None)
def pool_of(kind):
    if kind == 'runs':
        return Pool(8103, (300, 700), 400000, genome=RUNS)
    return {'short': Pool(8101, (300, 700), 400000), 'long': Pool(8102, (1500, 4000), 600000)}[kind]


class Cursor(object):
    """Reads of a pool one after the other, round and round."""

    def __init__(self, pool, start=0):
        self.pool, self.i = pool, start

    def take(self):
        r = self.pool.reads[self.i % len(self.pool.reads)]
        self.i += 1
        return r


class QuietCursor(Cursor):
    """... those only that stay clear of the genome's runs of GATCGATC..."""

    def take(self):
        while True:
            r = Cursor.take(self)
            lo, hi = int(r.pos.min()), int(r.pos.max()) + 8
            if (lo - 1) // RUN_EVERY == hi // RUN_EVERY and lo % RUN_EVERY > 4 * RUN_REPEATS:
                return r


def table_of(reads):
    cat = lambda name, dt: np.concatenate([getattr(r, name) for r in reads]).astype(dt)
    begin = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    n = len(reads)
    t = _lib.Table(cat('pos', np.int32), cat('ev', np.int32), cat('mu', np.int32), cat('idx', np.int32), cat('fl', np.uint8), begin,
                   np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32), n)
    return t, np.array([r.qual for r in reads], dtype=np.float64)


def prefix_of(table, qual, n_rows):
    """The first n_rows rows of a table (its last read cut short)."""
    n_seg = int(np.searchsorted(table.seg_row_begin, n_rows, side='left'))
    begin = np.concatenate([table.seg_row_begin[:n_seg], [n_rows]])
    t = _lib.Table(table.pos[:n_rows], None, None, table.event_idx[:n_rows], table.flags[:n_rows], begin, table.seg_read[:n_seg],
                   table.seg_contig[:n_seg], n_seg, evmu=table.evmu[:n_rows])
    return t, qual[:n_seg]


# ---------------------------------------------------------------------------------------------------
# the window machine, row by row, keeping the rows of every slot
# ---------------------------------------------------------------------------------------------------
class Rec(object):
    __slots__ = ('site', 'seg', 'rev', 'closer', 'slots')

    def __init__(self, site, seg, rev, closer, slots):
        self.site, self.seg, self.rev, self.closer, self.slots = site, seg, rev, closer, slots

    def rows(self):
        return [r for s in self.slots for r in s]

    def first_row(self):
        return min(self.rows())

    def last_row(self):
        return max(self.rows())

    def slot_rows(self, dst, k):
        """Rows of the slot that is printed at place dst of the record (:187-188)."""
        return self.slots[dst if self.rev else k - 1 - dst]


class Walk(object):
    def __init__(self, recs, f0):
        self.recs, self.f0 = recs, f0
        self.by_closer = {}
        for r in recs:
            self.by_closer.setdefault(r.closer, r)


def walk(table, ref, k, skip, tail=-1):
    """extract_contexts.py:147-291 over a table (no read is dropped for its quality) -> Walk: the flush records with the rows
    of their slots, and every read's first site row."""
    pos, fl, idx = table.pos.tolist(), table.flags.tolist(), table.event_idx.tolist()
    offs = ref.site_off(k)
    recs, f0 = [], [-1] * table.n_seg
    has, mpos, slots = False, 0, [[] for _ in range(k)]
    last_read, last_rev, last_seg, first_idx = -1, 0, -1, 0
    sb = table.seg_row_begin.tolist()
    for seg in range(table.n_seg):
        name = int(table.seg_read[seg])
        for r in range(sb[seg], sb[seg + 1]):
            ix = idx[r]
            if name != last_read:
                first_idx = ix
            f = fl[r]
            if f & N_FLAG:
                continue
            if name != last_read:
                rev = 0 if f & EQ_FLAG else 1
            else:
                rev = 0 if ix > first_idx else 1
            p = pos[r]
            off = offs[rev][p]
            if has and mpos != 0 and (name != last_read or p >= mpos + 1):
                recs.append(Rec(mpos, last_seg, last_rev, r, [list(s) for s in slots]))
                if off < 0 or name != last_read or p > mpos + skip + 1:
                    slots = [[] for _ in range(k)]
                    has = False
                else:
                    old, mpos = mpos, p + off
                    s = min(mpos - old, k)
                    slots = [[] for _ in range(s)] + slots[:k - s]
            if off >= 0:
                if has and mpos != 0:
                    if name != last_read:
                        has, slots = False, [[] for _ in range(k)]
                    elif rev != last_rev:
                        has = False
                if not (has and mpos != 0):
                    has, mpos = True, p + off
                if f0[seg] < 0:
                    f0[seg] = r
                last_read, last_rev, last_seg = name, rev, seg
                slots[off].append(r)
            elif has and mpos != 0:
                has, slots = False, [[] for _ in range(k)]
    if tail >= 0 and has and mpos != 0:
        recs.append(Rec(mpos, last_seg, last_rev, table.n_rows, [list(s) for s in slots]))
    return Walk(recs, f0)


def alone(read, ref, k, skip):
    """The walk over a read as a table of its own whose last window the next shard closes."""
    t, _ = table_of([read])
    return walk(t, ref, k, skip, tail=0)


def slot_values(table, rows):
    """fl((E4 - M4) / 1e4) of the rows, in row order (:286)."""
    rows = np.asarray(rows, dtype=np.int64)
    d = table.evmu[rows, 0].astype(np.int64) - table.evmu[rows, 1].astype(np.int64)
    return d.astype(np.float64) / 10000.0


# ---------------------------------------------------------------------------------------------------
# placing
# ---------------------------------------------------------------------------------------------------
class Claim(object):
    """kind: what lies on `row` (a table row); seg: the probe read; cut, offset: row == (a multiple of cut) + offset; more: what
    else the builder knows (per kind, see test_edge_tables.py)."""

    def __init__(self, kind, seg, row, cut, offset, **more):
        self.kind, self.seg, self.row, self.cut, self.offset, self.more = kind, seg, row, cut, offset, more
        if (row - offset) % cut:
            raise AssertionError('%s: row %d is not %+d from a multiple of %d' % (kind, row, offset, cut))

    def __repr__(self):
        return '%s at row %d = %d * %d %+d (read %d) %r' % (self.kind, self.row, (self.row - self.offset) // self.cut, self.cut,
                                                             self.offset, self.seg, self.more)


class EdgeTable(object):
    def __init__(self, name, motif, k, skip, table, qual, claims, tail=-1, rerun=False, unbroken=None):
        self.name, self.motif, self.k, self.skip, self.table, self.qual, self.claims = name, motif, k, skip, table, qual, claims
        self.tail, self.rerun, self.unbroken = tail, rerun, unbroken
        self.ref = ref_of(motif)

    def kind_is_regular(self):
        return not any(c.kind == 'violation' for c in self.claims)

    def describe(self, close_row):
        """The claims nearest to a record's close_row (for a failure's message)."""
        near = sorted(self.claims, key=lambda c: abs(c.row - close_row))[:2]
        return '%s [%s, k %d, skip %d, %d rows]; nearest claims: %s' % (self.name, self.motif, self.k, self.skip, self.table.n_rows, near)


class Builder(object):
    def __init__(self, cursor):
        self.cursor, self.reads, self.n = cursor, [], 0

    def add(self, read):
        """-> (segment, first row) of the read."""
        self.reads.append(read)
        self.n += len(read)
        return len(self.reads) - 1, self.n - len(read)

    def pad_to(self, row):
        if row < self.n:
            raise AssertionError('row %d lies behind the current row %d' % (row, self.n))
        while self.n < row:
            r = self.cursor.take()
            g = row - self.n
            self.add(r.cut(0, g) if len(r) > g else r)

    def place(self, items, tail_pad=300):
        """items: (target row, lead, emit, what) -- emit(builder, target) is called with the builder at row target - lead and
        returns claims.  Targets in ascending order; one that cannot be reached any more moves on by PERIOD."""
        heap = [(t, i, lead, emit) for i, (t, lead, emit) in enumerate(items)]
        heapq.heapify(heap)
        claims = []
        while heap:
            t, i, lead, emit = heapq.heappop(heap)
            if t - lead < self.n:
                heapq.heappush(heap, (t + PERIOD, i, lead, emit))
                continue
            self.pad_to(t - lead)
            claims += emit(self, t)
        self.pad_to(self.n + tail_pad)
        return claims

    def finish(self):
        return table_of(self.reads)


def targets(small=True):
    """[(row, offset, cuts)]: offsets -2 .. +2 from multiples 1, 2, 5 of 960, 1024 and 2048 and from 15360; -1, 0, +1 from 512 and 8 j.
    A row that is the same offset from several cuts (2048 = 2 * 1024) is one target with all of them."""
    out = [(c * m + o, c, o) for c in BIG_CUTS for m in MULTIPLES for o in OFFSETS]
    out += [(COINCIDE + o, c, o) for c in (PIECE, CHUNK) for o in OFFSETS]
    if small:
        out += [(c + o, STRIPE if c % 512 == 0 else UNIT, o) for c in SMALL_CUTS for o in (-1, 0, 1)]
    rows = {}
    for t, c, o in out:
        rows.setdefault((t, o), []).append(c)
    return [(t, o, cuts) for (t, o), cuts in sorted(rows.items())]


def _direct_records(w, n_rows, margin=2):
    """Records of a read alone that are closed inside it by the row directly behind their closing row."""
    return [r for r in w.recs if r.closer < n_rows - margin and r.rows() and r.closer == r.last_row() + 1 and r.first_row() >= 1]


class ProbeMaker(object):
    """Probes for one (motif, k, skip): pool reads cut around one of their windows and changed; every probe is analysed alone
    after the change, and a candidate whose event is not where it was meant to be is dropped for the next one."""

    def __init__(self, motif, k, skip, start=0):
        self.ref, self.k, self.skip = ref_of(motif), k, skip
        self.cur = Cursor(pool_of('short'), start)
        self._windows = []

    def window(self, room_behind=6, head=3):
        """-> (read cut to `head` rows in front of a window .. room_behind rows behind its closer, its record alone)."""
        for _ in range(2000):
            if not self._windows:
                r = self.cur.take()
                w = alone(r, self.ref, self.k, self.skip)
                self._windows = [(r, rec) for rec in _direct_records(w, len(r), margin=80)][:6]
                continue
            r, rec = self._windows.pop()
            a = rec.first_row() - head
            # (the head is cut at a row that is not filtered and in front of every row of the window)
            while a > 0 and (r.fl[a] & N_FLAG):
                a -= 1
            if a < 0 or (r.fl[a] & N_FLAG):
                continue
            b = min(len(r), rec.closer + 1 + room_behind)
            probe = r.cut(a, b)
            w = alone(probe, self.ref, self.k, self.skip)
            hit = [x for x in w.recs if x.site == rec.site and x.closer == rec.closer - a and x.slots == [[q - a for q in s] for s in rec.slots]]
            if hit:
                return probe, hit[0]
        raise AssertionError('no window found in the pool')

    def changed(self, change, check, **kw):
        """A window probe changed by change(probe, rec) -> new probe; check(walk, probe) -> the event or None."""
        for _ in range(300):
            probe, rec = self.window(**kw)
            new = change(probe, rec)
            if new is None:
                continue
            got = check(alone(new, self.ref, self.k, self.skip), new)
            if got is not None:
                return new, got
        raise AssertionError('no probe could be made')


# ---- event 1: the first row of a read ----
def start_tables(motif, k=6, skip=0):
    """One table per offset: a read starts at every target, behind a read that ends in (a) an ordinary row, (b) a site row
    whose window the new read's first row closes, (c) two or three filtered rows."""
    out = []
    for o in OFFSETS:
        pm = ProbeMaker(motif, k, skip, start=17 * (o + 3))
        ref = pm.ref
        items = []
        for (t, off, cuts) in targets():
            if off != o:
                continue
            for pred_kind in 'abc':
                def emit(b, t, pred_kind=pred_kind, cuts=cuts, off=off):
                    lead_rows = b.n
                    if pred_kind == 'a':
                        for _ in range(400):
                            r = pm.cur.take().cut(0, 16)
                            w = alone(r, ref, k, skip)
                            is_open = any(x.closer == len(r) for x in w.recs)
                            if not (r.fl[-1] & N_FLAG) and (motif == 'A' or not is_open):
                                break
                        else:
                            raise AssertionError('no ordinary read end found')
                        pred = r
                    elif pred_kind == 'b':
                        probe, rec = pm.window(head=24)
                        pred = probe.cut(0, rec.last_row() + 1 - (t % 2 if rec.last_row() - rec.first_row() >= 1 and not (probe.fl[rec.last_row() - 1] & N_FLAG) else 0))
                        pred = pred.cut(len(pred) - 16, len(pred)) if len(pred) > 16 else pred
                        w = alone(pred, ref, k, skip)
                        is_open = any(x.closer == len(pred) for x in w.recs)
                        if not is_open:
                            raise AssertionError('the read does not end in an open window')
                    else:
                        r = pm.cur.take().cut(0, 16)
                        pred = r.filtered(16 - 2 - t % 2, 16)
                        w = alone(pred, ref, k, skip)
                        is_open = any(x.closer == len(pred) for x in w.recs)
                    assert len(pred) == 16
                    ps, _ = b.add(pred)
                    s, row = b.add(pm.cur.take().cut(0, 10))
                    assert row == t and b.n - lead_rows == 26
                    return [Claim('start', s, t, cut, off, pred=pred_kind, pred_seg=ps, open=bool(is_open)) for cut in cuts]
                items.append((t, 16, emit))
        b = Builder(Cursor(pool_of('short'), 100 + 31 * (o + 3)))
        claims = b.place(items)
        table, qual = b.finish()
        out.append(EdgeTable('starts %+d' % o, motif, k, skip, table, qual, claims))
    return out


# ---- event 3 (and 2): the closing row of a window ----
def _closing_item(pm, t, cuts, off, j, tag=None):
    def change(probe, rec):
        return probe.with_filtered_behind(rec.last_row(), j)

    def check(w, new):
        for x in w.recs:
            if x.rows() and x.closer < len(new) and x.closer == x.last_row() + 1 + j and \
                    all(new.fl[q] & N_FLAG for q in range(x.last_row() + 1, x.closer)):
                return x
        return None
    probe, rec = pm.changed(change, check)
    e = rec.last_row()

    def emit(b, t):
        s, row = b.add(probe)
        assert row + e == t
        return [Claim('close', s, t, cut, off, behind=j, closer=t + 1 + j, first=row + rec.first_row(), tag=tag) for cut in cuts]
    return (t, e, emit)


def closing_tables(motif, k=6, skip=0):
    """One table per offset: a window's closing row on every target, its closer directly behind it and behind one, two and three
    filtered rows."""
    out = []
    for o in OFFSETS:
        pm = ProbeMaker(motif, k, skip, start=23 * (o + 3))
        items = [_closing_item(pm, t, cuts, off, j) for (t, off, cuts) in targets() if off == o for j in (0, 1, 2, 3)]
        b = Builder(Cursor(pool_of('short'), 200 + 37 * (o + 3)))
        claims = b.place(items)
        table, qual = b.finish()
        out.append(EdgeTable('closing rows %+d' % o, motif, k, skip, table, qual, claims))
    return out


def last_row_tables(motif, k=6, skip=0):
    """Tables of cut + offset rows whose last row is the closing row of a window that only the next shard closes: prefixes of one
    table per offset; every one is to be run with tail_contig -1 and 0."""
    out = []
    for o in OFFSETS:
        pm = ProbeMaker(motif, k, skip, start=29 * (o + 3))
        items = [_closing_item(pm, t - 1, cuts[:1], off - 1, 0, tag=(cuts, off)) for (t, off, cuts) in targets() if off == o]
        b = Builder(Cursor(pool_of('short'), 300 + 41 * (o + 3)))
        claims = b.place(items)
        table, qual = b.finish()
        for c in claims:
            n, (cuts, off) = c.row + 1, c.more['tag']
            pt, pq = prefix_of(table, qual, n)
            out.append(EdgeTable('last row: %d rows' % n, motif, k, skip, pt, pq,
                                 [Claim('last', pt.n_seg - 1, n, cut, off, first=c.more['first']) for cut in cuts], tail=0))
    return out


# ---- event 5: window lengths ----
WINDOW_LENGTHS = (31, 32, 33, 63, 64, 65, 66)


def window_tables(motif, k=6, skip=0):
    """Windows of exactly 31 .. 66 rows from their first to their closing row, the closing row on a cut (the window reaches
    length - 1 rows behind a piece's first row) and one row behind it."""
    out = []
    for o in (0, 1):
        pm = ProbeMaker(motif, k, skip, start=43 + 11 * o)
        items = []
        for n, length in enumerate(WINDOW_LENGTHS):
            for ci, cut in enumerate(BIG_CUTS):
                t = cut * MULTIPLES[(n + ci) % 3] + o

                def change(probe, rec, length=length):
                    have = rec.last_row() - rec.first_row() + 1
                    mid = [q for q in rec.rows() if q != rec.last_row()]
                    if have > length or not mid or not all(rec.slots):
                        return None
                    return probe.stalled(mid[len(mid) // 2], length - have + 1)

                def check(w, new, length=length):
                    for x in w.recs:
                        if all(x.slots) and x.closer < len(new) and x.last_row() - x.first_row() + 1 == length and x.closer == x.last_row() + 1:
                            return x
                    return None
                probe, rec = pm.changed(change, check)

                def emit(b, t, probe=probe, rec=rec, cut=cut, length=length):
                    s, row = b.add(probe)
                    assert row + rec.last_row() == t
                    return [Claim('window', s, t, cut, o, length=length, first=t - length + 1, closer=t + 1)]
                items.append((t, rec.last_row(), emit))
        b = Builder(Cursor(pool_of('short'), 400 + 47 * o))
        claims = b.place(items)
        table, qual = b.finish()
        out.append(EdgeTable('window lengths, closing row %+d' % o, motif, k, skip, table, qual, claims))
    return out


# ---- event 6: slot sizes ----
SLOT_SIZES = (7, 8, 9, 15, 16, 17, 127, 128)
SLOT_SIZES_REPEATED = (129, 257)         # a slot of more than 128 events marks a pipelined pass: it is repeated


def slot_tables(motif, k=6, skip=0):
    """A slot of exactly n events (one row of a window repeated n times), once clear of every cut and once with the repeated rows
    lying across a piece / chunk / tile cut.  Two tables: the sizes up to 128, and 129 / 257 (the pass is repeated)."""
    out = []
    for sizes, rerun in ((SLOT_SIZES, False), (SLOT_SIZES_REPEATED, True)):
        pm = ProbeMaker(motif, k, skip, start=59 + int(rerun))
        items = []
        for n, size in enumerate(sizes):
            for ci, cut in enumerate(BIG_CUTS + (None,)):
                def change(probe, rec, size=size):
                    ones = [s[0] for s in rec.slots if len(s) == 1]
                    if not ones or not all(rec.slots):
                        return None
                    change.row = ones[len(ones) // 2]
                    return probe.stalled(change.row, size)

                def check(w, new, size=size):
                    for x in w.recs:
                        if x.closer < len(new) and all(x.slots) and any(len(s) == size and s == list(range(change.row, change.row + size)) for s in x.slots):
                            return x
                    return None
                probe, rec = pm.changed(change, check)
                first = change.row
                i = [len(s) for s in rec.slots].index(size)
                dst = i if rec.rev else k - 1 - i
                if cut is None:                 # clear of the cuts: the whole probe between two of them
                    e, start = first, TILE * (9 + n) + 70
                    while any(start // c != (start + len(probe)) // c for c in BIG_CUTS):
                        start += 100
                    t = start + e
                else:
                    e = first + size // 2
                    t = cut * MULTIPLES[(n + ci) % 3]

                def emit(b, t, probe=probe, rec=rec, cut=cut, size=size, e=e, first=first, dst=dst):
                    s, row = b.add(probe)
                    assert row + e == t
                    return [Claim('slot', s, t, cut or 1, 0, size=size, across=cut is not None, first=row + first, closer=row + rec.closer, dst=dst)]
                items.append((t, e, emit))
        b = Builder(Cursor(pool_of('short'), 500 + int(rerun)))
        claims = b.place(items)
        table, qual = b.finish()
        out.append(EdgeTable('slot sizes %s' % (sizes,), motif, k, skip, table, qual, claims, rerun=rerun))
    return out


# ---- event 7: gaps of filtered rows across a cut ----
GAP_LENGTHS = (1, 2, 3, 31, 32, 63, 64, 65)


def gap_tables(motif, k=6, skip=0):
    """Gaps of filtered rows behind a window's closing row that begin before a cut and end behind it: the closing row and the
    closer lie on different sides of the cut, up to 65 rows apart."""
    pm = ProbeMaker(motif, k, skip, start=71)
    items = []
    for n, L in enumerate(GAP_LENGTHS):
        for a in ((0, 1) if L == 1 else (1, L // 2, L - 1) if L > 3 else (1, L - 1) if L == 3 else (1,)):
            for ci, cut in enumerate(BIG_CUTS):
                def change(probe, rec, L=L):
                    if len(probe) < rec.closer + L + 2:
                        return None
                    return probe.filtered(rec.closer, rec.closer + L)

                def check(w, new, L=L):
                    for x in w.recs:
                        if x.rows() and x.closer < len(new) and x.closer - x.last_row() - 1 == L and \
                                all(new.fl[q] & N_FLAG for q in range(x.last_row() + 1, x.closer)):
                            return x
                    return None
                probe, rec = pm.changed(change, check, room_behind=L + 8)
                e = rec.last_row() + 1 + a
                t = cut * MULTIPLES[(n + ci + a) % 3]

                def emit(b, t, probe=probe, rec=rec, cut=cut, L=L, a=a, e=e):
                    s, row = b.add(probe)
                    assert row + e == t
                    return [Claim('gap', s, t, cut, 0, length=L, before=a, closing=row + rec.last_row(), closer=row + rec.closer)]
                items.append((t, e, emit))
    b = Builder(Cursor(pool_of('short'), 600))
    claims = b.place(items)
    table, qual = b.finish()
    return [EdgeTable('gaps of filtered rows', motif, k, skip, table, qual, claims)]


# ---- event 4: the first site row of a block ----
F0_OFFSETS = (0, 1, 511, 512, 513, 1023, 1024)
NO_SITE_BLOCKS = (512, 513)


def first_site_of_block(table, ref, k, seg):
    """The block's first row whose k-mer covers a marked position on its strand, from the flags and the marked strings alone
    (the strand of a row in front of the first site row: '+' iff its model k-mer is the reference's, :169-174); -1 if none."""
    for r in range(int(table.seg_row_begin[seg]), int(table.seg_row_begin[seg + 1])):
        f = int(table.flags[r])
        if f & N_FLAG:
            continue
        p = int(table.pos[r])
        if ref.marked[0 if f & EQ_FLAG else 1][p:p + k].any():
            return r
    return -1


def first_site_tables(motif, k=6, skip=0):
    """Blocks whose first site row lies 0, 1, 511, 512, 513, 1023 and 1024 rows behind their first row (sparse motif: a stretch
    of a read that holds no site; one-base motif: filtered rows in front), blocks of exactly 512 and 513 rows without any, and a
    reverse read whose first site row is palindromic (R5) at offsets 0 and 1.  The blocks start on rows around the cuts."""
    ref = ref_of(motif)
    offs = ref.site_off(k)
    dense = len(motif) == 1
    cur = Cursor(pool_of('short' if dense else 'long'), 5)
    starts = iter([PIECE - 1, CHUNK * 2, TILE * 2 + 1, PIECE * 5, CHUNK * 5 - 1, TILE * 5, COINCIDE, PERIOD + PIECE, PERIOD + CHUNK, PERIOD + TILE + 1,
                   PERIOD + 2 * TILE, PERIOD + 5 * PIECE + 1, PERIOD + 5 * CHUNK, PERIOD + 5 * TILE - 1])

    def site_rows(r):
        rev = 0 if r.up() else 1
        return [i for i in range(len(r)) if not (r.fl[i] & N_FLAG) and offs[rev][int(r.pos[i])] >= 0]

    def block(d, palindromic=False, none=0):
        for _ in range(3000):
            r = cur.take()
            if dense and not palindromic:
                n = none or d + 40
                if len(r) < n + 1:
                    continue
                probe = r.cut(0, n)
                probe = probe.filtered(0, n if none else d)
            else:
                sites = site_rows(r)
                probe = None
                if palindromic:
                    if r.up():
                        continue
                    pal = [i for i in range(len(r)) if (r.fl[i] & EQ_FLAG) and offs[0][int(r.pos[i])] >= 0 and i >= d]
                    for i in pal:
                        probe = r.cut(i - d, min(len(r), i + 40))
                        if alone(probe, ref, k, skip).f0[0] == d:
                            break
                        probe = None
                else:
                    for a, z in zip([-1] + sites, sites + [len(r)]):
                        if none and z - a - 1 >= none + 2:
                            probe = r.cut(a + 1, a + 1 + none)
                        elif not none and z < len(r) and z - a - 1 >= d:
                            probe = r.cut(z - d, min(len(r), z + 40))
                        if probe is not None and (probe.fl[0] & N_FLAG):
                            probe = None
                        if probe is not None:
                            break
                if probe is None:
                    continue
            f0 = alone(probe, ref, k, skip).f0[0]
            if f0 == (-1 if none else d) and (not palindromic or (probe.fl[d] & EQ_FLAG and not probe.up())):
                return probe
        raise AssertionError('no block with its first site row at %d found' % d)

    items = []
    for d, pal, none in [(d, False, 0) for d in F0_OFFSETS] + [(0, False, n) for n in NO_SITE_BLOCKS] + [(0, True, 0), (1, True, 0)]:
        probe = block(d, pal, none)
        t = next(starts)

        def emit(b, t, probe=probe, d=d, pal=pal, none=none):
            s, row = b.add(probe)
            assert row == t
            return [Claim('f0', s, t + d if not none else t, 1, 0, block_offset=-1 if none else d, block_rows=len(probe), palindromic=pal)]
        items.append((t, 0, emit))
    b = Builder(Cursor(pool_of('short'), 700))
    claims = b.place(items)
    table, qual = b.finish()
    return [EdgeTable('first site rows', motif, k, skip, table, qual, claims)]


# ---- event 8: a violation that one pair of rows shows ----
VIOLATION_CUTS = (8, 24, 512, 960, 1024, 2048)


def violation_tables(motif, k=6, skip=0):
    """One table per (cut, pair, kind): a read that looks regular on its first rows and whose single offending pair of rows --
    the position going back by one ('pos'), equal event indices ('idx') -- is (cut - 1, cut), the pair before it or the pair
    behind it.  'pos' pairs lie inside a window and change the records (EdgeTable.unbroken: the same table without the
    violation); every table's first pass must be repeated."""
    ref = ref_of(motif)
    out = []
    pm = ProbeMaker(motif, k, skip, start=83)
    for cut in VIOLATION_CUTS:
        for d in (-1, 0, 1):
            for kind in ('pos', 'idx'):
                target = cut + d                     # the second row of the pair
                for _ in range(200):
                    probe, rec = pm.window(room_behind=12)
                    rows = sorted(rec.rows())
                    # the second row of the pair: the closing row or the row before it, both rows of the pair in the window
                    e = rows[-1] if (cut + d) % 2 else (rows[-2] if len(rows) > 1 else rows[-1])
                    if e < 1 or e - 1 not in rows:
                        continue
                    broken = probe.cut(0, len(probe))
                    if kind == 'pos':
                        if broken.pos[e - 1] < 2:
                            continue
                        broken.pos[e] = broken.pos[e - 1] - 1
                    else:
                        broken.idx[e] = broken.idx[e - 1]
                    if kind == 'pos':
                        wa, wb = alone(probe, ref, k, skip), alone(broken, ref, k, skip)
                        # (what a record shows of its slots: their means, unless it has too many empty ones)
                        sig = lambda w: [(x.site, x.closer, x.slots if sum(not q for q in x.slots) <= skip else None) for x in w.recs]
                        if sig(wa) == sig(wb):
                            continue
                    break
                else:
                    raise AssertionError('no probe whose records the violation changes')
                if e > target:                       # (a window does not fit in front of the row: the same residues a period on)
                    target += PERIOD
                tables = []
                for p in (broken, probe):
                    b = Builder(Cursor(pool_of('short'), 800 + cut % 97 + d))
                    b.pad_to(target - e)
                    s, row = b.add(p)
                    b.pad_to(b.n + 150)
                    tables.append(b.finish())
                c = Claim('violation', s, target, STRIPE if cut == 512 else UNIT if cut < 512 else cut, d, what=kind, pair=(target - 1, target))
                out.append(EdgeTable('violation %s at (%d, %d)' % (kind, target - 1, target), motif, k, skip, tables[0][0], tables[0][1], [c],
                                     rerun=True, unbroken=tables[1][0]))
    return out


# ---- event 10: name blocks per chunk / per staged range ----
def block_count_tables(motif, k=6, skip=0):
    """Exactly 2, 3 and 4 name blocks in one 1024-row chunk of the scan; exactly 16, 17 and 18 in the rows a piece of k1_fused
    stages (64 rows in front of its 960) and in those a piece of k1_emit_runs stages (128 in front of its 1024)."""
    cur = Cursor(pool_of('short'), 900)
    b = Builder(cur)
    claims = []

    def blocks_in(lo, hi, n, what, cut):
        """Exactly n blocks overlap rows [lo, hi): one that begins in front of lo, n - 1 that begin inside, the last reaching hi."""
        assert b.n < lo
        b.pad_to(lo - 5)
        step = (hi - lo) // n
        for i in range(n):
            end = hi + 5 if i == n - 1 else lo + step * (i + 1)
            r = cur.take()
            while len(r) < end - b.n:
                r = cur.take()
            s, row = b.add(r.cut(0, end - b.n))
        claims.append(Claim('blocks', s, lo, cut, 0, lo=lo, hi=hi, n=n, what=what))

    for n in (2, 3, 4):
        c = 2 + 2 * (n - 2)
        blocks_in(CHUNK * c, CHUNK * (c + 1), n, 'scan chunk', CHUNK)
    for n in (F_MAXB, F_MAXB + 1, F_MAXB + 2):
        p = 10 + 2 * (n - F_MAXB)
        blocks_in(PIECE * p - FH, PIECE * (p + 1), n, 'fused piece', 1)
    for n in (E_MAXB, E_MAXB + 1, E_MAXB + 2):
        p = 18 + 2 * (n - E_MAXB)
        blocks_in(ET * p - EH, ET * (p + 1), n, 'emit_runs piece', 1)
    b.pad_to(b.n + 300)
    table, qual = b.finish()
    return [EdgeTable('name blocks per chunk / piece', motif, k, skip, table, qual, claims)]


# ---- event 9: more closing rows in a tile than it has payload slots of its own ----
def tile_count_tables(motif, k=6, skip=0):
    """Exactly PT, PT + 1 and PT + 2 closing rows in one tile of the scan under a sparse motif: a read across a run of GATCGATC...
    in the genome, cut off behind as many of the run's windows as the tile still needs (counted by the walk over the tile's reads)."""
    assert motif.endswith(RUNS)
    ref = ref_of(motif)
    # (the library takes a reference with more than one marked position in 64 bases, both strands counted, for a dense one)
    assert int(ref.marked[0].sum() + ref.marked[1].sum()) * 64 < GENOME_LEN, 'the runs make the reference a dense one'
    cur = Cursor(pool_of('runs'), 3)
    b = Builder(QuietCursor(pool_of('short'), 501))
    claims = []
    for i, want in enumerate((PT, PT + 1, PT + 2)):
        t0 = TILE * (2 + 2 * i)
        b.pad_to(t0 - 100)
        b.pad_to(t0 + 40)                                   # (a read of its own across the tile's first row)
        keep = (len(b.reads), b.n, b.cursor.i)
        first_read = keep[0] - 1
        base = b.n - len(b.reads[-1])

        def closing_rows_in_the_tile():
            t, _ = table_of(b.reads[first_read:])
            return sum(1 for x in walk(t, ref, k, skip).recs if x.rows() and t0 <= base + x.last_row() < t0 + TILE)
        done = False
        for _ in range(1500):
            r = cur.take()
            w = alone(r, ref, k, skip)
            recs = [x for x in w.recs if x.rows() and x.closer < len(r)]
            # the first stretch of windows that follow each other within twenty rows: the read's way across a run
            near = [j for j in range(1, len(recs)) if recs[j].last_row() - recs[j - 1].last_row() <= 20]
            dense = [j for n, j in enumerate(near) if j == near[0] + n]
            if len(dense) < PT + 2 or recs[dense[0] - 1].first_row() < 6:
                continue
            a = recs[dense[0] - 1].first_row() - 5
            if r.fl[a] & N_FLAG:
                continue
            for j in [dense[0] - 1] + dense:
                b.add(r.cut(a, recs[j].closer + 2))
                s = len(b.reads) - 1
                b.pad_to(t0 + TILE + 100)
                if closing_rows_in_the_tile() == want:
                    done = True
                    break
                del b.reads[keep[0]:]
                b.n, b.cursor.i = keep[1], keep[2]
            if done:
                break
        if not done:
            raise AssertionError('no read gives tile %d exactly %d closing rows' % (t0 // TILE, want))
        claims.append(Claim('tile', s, t0, TILE, 0, n=want))
    b.pad_to(b.n + 300)
    table, qual = b.finish()
    return [EdgeTable('closing rows per tile', motif, k, skip, table, qual, claims)]


MAKERS = {'start': start_tables, 'close': closing_tables, 'last': last_row_tables, 'window': window_tables, 'slot': slot_tables,
          'gap': gap_tables, 'f0': first_site_tables, 'violation': violation_tables, 'blocks': block_count_tables, 'tile': tile_count_tables}


@functools.lru_cache(maxsize=None)
def tables(kind, motif, k=6, skip=0):
    return MAKERS[kind](motif, k, skip)
