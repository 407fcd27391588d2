"""Site cases: small, seeded, hand-placed inputs for the per-site reduction (k_site_counts and the mc_site_counts* calls of
mc_stream.hip, mc_site_allreduce of mc_comm.hip) with the reduction they must give.  TEST INFRASTRUCTURE:
tests/test_site_cases.py holds every claim made here on the CPU, tests/test_gpu_site_counts.py runs the cases on the device.

A case is a FASTA of several contigs, a marking of it, an event table whose reads are laid over chosen spans of the contigs,
read qualities, and the EXPECTED reduction.  The expectation is a plain restatement that shares nothing with
make_bed.site_counts or SiteIndex: a Python loop over the C oracle's flush records fills a dict keyed (contig of the site,
strand, position) with [n_meth, n_total, smallest closing row + row_offset]; a second loop walks the marked strings in
(contig, strand, position) order and hands out the site numbers.

The sites are chosen for where the numbering can go wrong: mask bits 0, 31, 32, 63 and 64 of a contig, the last scoreable
position L - k, contigs of 31, 32, 33, 64 and 65 bases, one shorter than k, one without a site on one strand, one without any
site between two that have some, a position marked on both strands (an 'M' in the FASTA itself), sites within k of a contig
end (MC_I_EDGE: the device leaves them to the host), a site under 300 reads, a site under one and under none; the tables for
where the choice of records and table can go wrong: windows closed by the first row of a read on another contig, a table
that ends in an open window, a read with a position stepping back (the literal path), a read with a gap (MC_I_TOO_MANY), and
two tables A and B whose segments map to different contigs."""
import functools
import os

import numpy as np

from mcaller_amd import _lib, refmark
from tests import helpers as H

K, SKIP = 6, 1                 # (skip_thresh 1: a window may lack one position -- the one beyond a contig's end)
ROW_REACH = 6                  # a row's model k-mer: an eventalign row sits at most L - 6 on a contig of L bases
INT64_MAX = int(np.iinfo(np.int64).max)
BIG_OFFSET = 3 << 40           # a row offset beyond 32 bits (multi_gpu: rank * ROW_STRIDE)

# name, length, '+' marks, '-' marks, (start, letters) planted for the motif and IUPAC markings.  A position marked on both
# strands is an 'M' in the FASTA, '+' only an 'A', '-' only a 'T'; the rest is seeded (`empty` and `ballast`: C and G only -- no
# marking finds a site on them).
CONTIGS = (
    ('len31', 31, (5, 25), (4, 12, 26), ((8, 'GATC'),)),
    ('len32', 32, (4, 27), (26,), ((20, 'GATC'),)),
    ('len33', 33, (0, 10, 27), (), ((28, 'GATC'),)),
    ('tiny', 4, (1,), (2,), ()),
    ('len64', 64, (5, 31, 40, 58), (32, 40, 59), ((30, 'GATC'),)),
    ('empty', 40, (), (), ()),
    ('len65', 65, (5, 31, 60), (4, 32, 59), ((30, 'GATC'),)),
    ('long', 400, (63, 127, 128, 180, 220, 250, 300, 393), (31, 32, 64, 95, 96, 180, 340, 394),
     ((62, 'GATC'), (140, 'GATC'), (299, 'GACTC'), (392, 'GATC'))),
    ('twin1', 80, (20, 40, 70), (30,), ((50, 'GATC'), (74, 'GATC'))),
    ('twin2', 80, (20, 40, 70), (30,), ((50, 'GATC'), (74, 'GATC'))),
    # (bases without a site: the library takes a reference with more than one site in 64 bases for a dense one, whose pipelined
    # passes run as k1_fused -- that is the dense case's business)
    ('ballast', 4000, (), (), ()),
)
C_LEN31, C_LEN32, C_LEN33, C_TINY, C_LEN64, C_EMPTY, C_LEN65, C_LONG, C_TWIN1, C_TWIN2, C_BALLAST = range(11)
MOTIF = 'GATC'
IUPAC = 'GATC:2,GANTC:2'
CROWD = 300                    # reads over the crowded site
CROWDED, ONCE, NEVER = (C_LONG, 0, 220), (C_LONG, 0, 250), (C_LONG, 0, 300)
BOTH = ((C_LONG, 180), (C_LEN64, 40))          # positions marked on both strands that reads of both strands cover
DENSE_CONTIGS = (('dense1', 2500), ('dense2', 1200), ('dense3', 33))


@functools.lru_cache(maxsize=None)
def weights():
    from mcaller_amd import rows
    _, w, _, soc = rows.submodel_setup(H.load_modelset('r95'), 'A')
    return w, soc


# ---------------------------------------------------------------------------------------------------
# the FASTA, the reads, the table
# ---------------------------------------------------------------------------------------------------
def placed_sequences():
    rng = np.random.default_rng(6021)
    out = []
    for name, length, fwd, rev, planted in CONTIGS:
        letters = 'CG' if name in ('empty', 'ballast') else 'ACGT'
        seq = [letters[i] for i in rng.integers(0, len(letters), length)]
        fixed = {}
        for at, text in planted:
            for i, ch in enumerate(text):
                fixed[at + i] = ch
        for p in set(fwd) | set(rev):
            ch = 'M' if (p in fwd and p in rev) else ('A' if p in fwd else 'T')
            if fixed.get(p, ch) != ch:
                raise AssertionError('%s: position %d is planted %s and marked %s' % (name, p, fixed[p], ch))
            fixed[p] = ch
        for p, ch in fixed.items():
            seq[p] = ch
        out.append((name, ''.join(seq)))
    # (the twins: one sequence, so that a record counted on the wrong one of them still names a marked site)
    out[C_TWIN2] = (out[C_TWIN2][0], out[C_TWIN1][1])
    return out


def dense_sequences():
    rng = np.random.default_rng(6022)
    return [(name, ''.join('ACGT'[i] for i in rng.integers(0, 4, length))) for name, length in DENSE_CONTIGS]


def write_fasta(path, sequences):
    with open(path, 'w') as fh:
        for name, seq in sequences:
            fh.write('>%s\n' % name)
            for i in range(0, len(seq), 60):
                fh.write(seq[i:i + 60] + '\n')


def write_positions(path):
    with open(path, 'w') as fh:
        for name, _, fwd, rev, _ in CONTIGS:
            for p in fwd:
                fh.write('%s\t%d\t+\tm6A\n' % (name, p))
            for p in rev:
                fh.write('%s\t%d\t-\tm6A\n' % (name, p))


class Read(object):
    """One read: rows over positions [a, b) of a contig in ascending order, one or two rows a position; drop: positions left
    out (a gap); back_at: the rows step back by one position once, behind position back_at."""

    def __init__(self, contig, a, b, rev, drop=(), back_at=None):
        self.contig, self.a, self.b, self.rev, self.drop, self.back_at = contig, a, b, bool(rev), tuple(drop), back_at


def make_table(reads, lengths, seed):
    rng = np.random.default_rng(seed)
    cols = dict(pos=[], ev=[], mu=[], idx=[], fl=[])
    begin, contigs = [0], []
    for r in reads:
        if not (0 <= r.a < r.b and r.b - 1 <= lengths[r.contig] - ROW_REACH):
            raise AssertionError('a read over [%d, %d) does not fit contig %d' % (r.a, r.b, r.contig))
        where = []
        for p in range(r.a, r.b):
            if p in r.drop:
                continue
            where.append(p)
            if p == r.back_at:
                where += [p - 1, p]
        where = np.array(where, dtype=np.int64)
        pos = np.repeat(where, 1 + (rng.random(len(where)) < 0.3))
        n = len(pos)
        mu = 550000 + ((pos * 7919 + r.contig * 104729 + int(r.rev) * 31337) % 6200) * 100
        ev = mu + np.round(rng.normal(-0.17, 2.44, n) * 100).astype(np.int64) * 100
        i0 = int(rng.integers(0, 50000))
        idx = i0 + n - np.arange(n) if r.rev else i0 + np.arange(n)
        fl = np.zeros(n, dtype=np.uint8)
        if not r.rev:
            fl |= np.uint8(_lib.F_KMER_EQ)
        fl[0] |= _lib.F_SEG_START | _lib.F_NAME_START
        for name, col in zip(('pos', 'ev', 'mu', 'idx', 'fl'), (pos, ev, mu, idx, fl)):
            cols[name].append(col)
        begin.append(begin[-1] + n)
        contigs.append(r.contig)
    n = len(reads)
    cat = lambda name, dt: np.concatenate(cols[name]).astype(dt) if n else np.zeros(0, dt)      # noqa: E731
    table = _lib.Table(cat('pos', np.int32), cat('ev', np.int32), cat('mu', np.int32), cat('idx', np.int32), cat('fl', np.uint8),
                       np.array(begin, dtype=np.int64), np.arange(n, dtype=np.int32), np.array(contigs, dtype=np.int32), n,
                       read_names=['site-case-%d-read-%05d' % (seed, i) for i in range(n)])
    return table, np.round(rng.uniform(6.0, 12.0, n), 3)


def whole(contig, rev, length, a=0):
    return Read(contig, a, length - ROW_REACH + 1, rev)


def placed_reads(irregular=False):
    """The reads of the hand-placed table.  Every contig of 31 bases and more: reads of both strands over the whole contig, twice
    -- a window that the read's last row leaves open (a site at L - k or L - k + 1: the row that would close it does not exist) is
    closed by the first row of the next read, of the same contig but for the last read."""
    lengths = [c[1] for c in CONTIGS]
    reads = []
    for c in (C_LEN31, C_LEN32, C_LEN33, C_LEN64):
        # (no row on position 0 of len33, which is marked: a site at 0 is never flushed, a read that lies on it goes through the
        # literal path, and what its rows leave in the slots is not the business of these cases)
        reads += [whole(c, rev, lengths[c], a=1 if c == C_LEN33 else 0) for rev in (0, 1, 1, 0)]
    # the named cross-contig record: '+' 58 of len64, its position L - k, left open by a read of len64 and closed by the first row
    # of a read on `empty`; counted before, from the reads that a read of len64 closes
    reads += [Read(C_LEN64, 50, 59, 0), whole(C_EMPTY, 0, lengths[C_EMPTY]), whole(C_EMPTY, 1, lengths[C_EMPTY])]
    reads += [whole(C_LEN65, rev, lengths[C_LEN65]) for rev in (0, 1, 0, 1)]
    # `long`: everything but position 300, position 250 once
    reads += [Read(C_LONG, 50, 290, 0), Read(C_LONG, 20, 200, 1), Read(C_LONG, 380, 395, 0), Read(C_LONG, 330, 360, 1),
              Read(C_LONG, 50, 240, 0), Read(C_LONG, 380, 395, 1), Read(C_LONG, 20, 110, 1)]
    if irregular:
        reads.append(Read(C_LONG, 55, 75, 0, back_at=61))
    # a gap at 125 and 126: the windows of 127 and 128 have two empty slots (MC_I_TOO_MANY at skip_thresh 1)
    reads.append(Read(C_LONG, 116, 136, 0, drop=(125, 126)))
    reads += [Read(C_LONG, 214, 224, 0) for _ in range(CROWD)]
    reads += [Read(C_TWIN1, 10, 75, 0), Read(C_TWIN2, 10, 75, 1)]
    # the table ends in an open window: '-' 394 of `long`, its last scoreable position
    reads.append(Read(C_LONG, 385, 395, 1))
    return reads


def interior_reads():
    """Reads for the motif table: clear of the contig ends (no MC_I_EDGE record: every record is a row of the .diffs text),
    and '-' reads that leave the window of 394 on `long` to the first row of another contig's read or to the table's end."""
    lengths = [c[1] for c in CONTIGS]
    reads = []
    for c in (C_LEN31, C_LEN32, C_LEN33, C_LEN64, C_EMPTY, C_LEN65, C_LONG, C_TWIN1, C_TWIN2):
        a, b = K - 1, lengths[c] - 2 * K + 2
        for rev in (0, 1, 0, 1):
            reads.append(Read(c, a, b, rev))
        if c in (C_LEN64, C_LEN65):
            reads.append(Read(C_LONG, 380, 395, 1))
    reads += [Read(C_LONG, 130, 150, rev) for rev in (0, 1) * 10]
    reads.append(Read(C_LONG, 385, 395, 1))
    return reads


def edge_to_edge_reads():
    """Reads for the IUPAC table: whole contigs, both strands, twice."""
    lengths = [c[1] for c in CONTIGS]
    reads = []
    for c in (C_LEN31, C_LEN32, C_LEN33, C_LEN64, C_EMPTY, C_LEN65, C_LONG, C_TWIN1, C_TWIN2):
        reads += [whole(c, rev, lengths[c]) for rev in (0, 1, 1, 0)]
    reads.append(Read(C_LONG, 385, 395, 1))
    return reads


def twin_reads(which):
    """Tables A and B: the same kinds of reads on the twins, mapped to them the other way round and cut differently."""
    x, y = (C_TWIN1, C_TWIN2) if which == 'A' else (C_TWIN2, C_TWIN1)
    if which == 'A':
        reads = [Read(x, 10, 50, 0), Read(x, 60, 71, 0), Read(y, 10, 50, 0), Read(y, 60, 71, 0), Read(x, 20, 40, 1), Read(y, 60, 71, 0),
                 Read(y, 15, 45, 1), Read(x, 60, 71, 0), Read(x, 12, 30, 0), Read(y, 60, 71, 0)]
    else:
        reads = [Read(x, 60, 71, 0), Read(x, 10, 50, 0), Read(x, 60, 71, 0), Read(y, 10, 50, 0), Read(y, 20, 40, 1), Read(x, 60, 71, 0),
                 Read(x, 15, 45, 1), Read(y, 12, 30, 0), Read(y, 60, 71, 0), Read(y, 10, 50, 0), Read(x, 60, 71, 0), Read(x, 10, 50, 1),
                 Read(y, 60, 71, 0)]
    return reads


def dense_reads():
    rng = np.random.default_rng(6023)
    reads = []
    for c, (_, length) in enumerate(DENSE_CONTIGS):
        top = length - ROW_REACH + 1
        if top < 100:
            reads += [Read(c, 1, top, rev) for rev in (0, 1, 0)]
            continue
        reads += [Read(c, 1, 150, 0), Read(c, 1, 150, 1)]          # (from 1: a read on a marked position 0 takes the literal path)
        for _ in range(length // 70):
            n = int(rng.integers(60, 400))
            a = int(rng.integers(1, top - n))
            reads.append(Read(c, a, a + n, int(rng.integers(0, 2))))
        reads += [Read(c, top - 150, top, 1), Read(c, top - 150, top, 0)]
    reads.append(Read(0, 2300, 2495, 0))                # (the table ends in an open window)
    return reads


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
class Expected(object):
    """n_meth, n_total (int32 per site), first (int64 per site, INT64_MAX where n_total is 0); pending: records the device leaves
    to the host (NaN probability there), counted here like the others; n_cross: records closed by another contig's row, left out;
    extras: their BED rows; counted: the dict; unmarked: records that name no marked site (a wrong table only)."""


def number_the_sites(meth, n_contigs):
    """{(contig, strand, position): site number} in (contig, strand, position) order, from the marked strings."""
    number = {}
    for c in range(n_contigs):
        for strand in (0, 1):
            for p, ch in enumerate(meth[c][strand]):
                if ch == 'M':
                    number[(c, strand, p)] = len(number)
    return number


def restate(rec, prob, nan, table, meth, names, n_contigs, k, tail_contig=-1, row_offset=0, device_only=False):
    """The reduction of the records `rec` (probabilities `prob`; nan: the records the device does not score) on `table`;
    device_only: without the records left to the host -- the counts before they have been added."""
    seg_of_row = []
    for s in range(table.n_seg):
        seg_of_row += [s] * (int(table.seg_row_begin[s + 1]) - int(table.seg_row_begin[s]))
    counted, cross, extras, pending, unmarked = {}, [], [], 0, 0
    number = number_the_sites(meth, n_contigs)
    for j in range(rec.n):
        info = int(rec.info[j])
        if info & _lib.I_TOO_MANY:
            continue
        contig = int(table.seg_contig[int(rec.site_seg[j])])
        rev = 1 if info & _lib.I_REV else 0
        pos, row = int(rec.site_pos[j]), int(rec.close_row[j])
        closer = int(table.seg_contig[seg_of_row[row]]) if row < len(seg_of_row) else tail_contig
        is_meth = bool(prob[j] >= 0.5)
        if closer != contig:
            cross.append(j)
            context = refmark.revcomp(meth[contig][rev][pos - k + 1:pos + k], bool(rev))
            extras.append((names[closer], pos, '-' if rev else '+', context, is_meth, row + row_offset))
            continue
        if (contig, rev, pos) not in number:
            unmarked += 1
            continue
        pending += 1 if nan[j] else 0
        if nan[j] and device_only:
            continue
        e = counted.setdefault((contig, rev, pos), [0, 0, row + row_offset])
        e[0] += 1 if is_meth else 0
        e[1] += 1
        e[2] = min(e[2], row + row_offset)
    x = Expected()
    x.n_sites = len(number)
    x.n_meth, x.n_total = np.zeros(x.n_sites, dtype=np.int32), np.zeros(x.n_sites, dtype=np.int32)
    x.first = np.full(x.n_sites, INT64_MAX, dtype=np.int64)
    for key, (m, t, f) in counted.items():
        x.n_meth[number[key]], x.n_total[number[key]], x.first[number[key]] = m, t, f
    x.counted, x.number, x.pending, x.n_cross, x.cross, x.extras, x.unmarked = counted, number, pending, len(cross), cross, extras, unmarked
    return x


def stand_in(j):
    """What the host's scoring of a record the device leaves to it is taken to be: both labels occur."""
    return 0.75 if j % 3 else 0.25


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
class Case(object):
    """name; setter: how the reference goes to the device ('masks': set_reference with the host's marking, 'motif':
    set_reference_motif, 'iupac': set_reference_iupac -- the masks, the rank arrays and site_base made on the device); tail: the
    tail_contig the table is meant to be run with."""

    def __init__(self, name, ref, setter, table, qual, tail):
        self.name, self.ref, self.setter, self.table, self.qual, self.tail = name, ref, setter, table, qual, tail
        self.k, self.skip = K, SKIP
        self.n_contigs = len(ref.names)
        self.lengths = [len(seq) for _, seq in ref.records]
        self._records = {}

    def set_reference(self, dev):
        if self.setter == 'motif':
            dev.set_reference_motif(self.ref.raw_arrays(), *self.ref.motif_for_the_device())
        elif self.setter == 'iupac':
            dev.set_reference_iupac(self.ref.raw_arrays(), self.ref.iupac_for_the_device())
        else:
            dev.set_reference(self.ref.device_arrays())

    def records(self, tail=None, model=None):
        """(the oracle's records, the probability of every record, which of them the device does not score); model: a classifier
        other than the r95 MLP, (weights, submodel of char)."""
        tail = self.tail if tail is None else tail
        key = (tail, id(model))
        if key not in self._records:
            w, soc = model or weights()
            rec = H.oracle_records(self.table, self.ref.device_arrays(), self.qual, self.k, self.skip, 0.0, tail_contig=tail)
            H.oracle_score(rec, self.table, self.qual, w, soc, self.k)
            prob = np.array(rec.prob[:rec.n], dtype=np.float64)
            nan = np.isnan(prob)
            for j in np.flatnonzero(nan):
                prob[j] = stand_in(int(j))
            self._records[key] = (rec, prob, nan, model)
        return self._records[key][:3]

    def expected(self, tail=None, row_offset=0, table=None, model=None, device_only=False, meth=None):
        """The restatement; table: the table whose segments and rows the records are looked up in (default: the case's own)."""
        tail = self.tail if tail is None else tail
        rec, prob, nan = self.records(tail, model)
        return restate(rec, prob, nan, table or self.table, meth or self.ref.meth, self.ref.names, self.n_contigs, self.k, tail, row_offset,
                       device_only)

    def marked(self, contig, rev, pos):
        return self.ref.meth[contig][rev][pos] == 'M'


def add(a, b):
    """Two reductions over the same sites, one after the other."""
    x = Expected()
    x.n_sites = a.n_sites
    x.n_meth, x.n_total, x.first = a.n_meth + b.n_meth, a.n_total + b.n_total, np.minimum(a.first, b.first)
    return x


def _marked_reference(fasta, motif, positions):
    ref = refmark.MarkedReference(fasta, 'A', motif, positions)
    for c in range(len(ref.names)):
        ref.mark(c)
    return ref


@functools.lru_cache(maxsize=None)
def cases(directory):
    """Every case, its files written into `directory` -> {name: Case}."""
    fasta, positions, dense_fasta = (os.path.join(directory, n) for n in ('sites.fasta', 'sites.positions.txt', 'dense.fasta'))
    write_fasta(fasta, placed_sequences())
    write_positions(positions)
    write_fasta(dense_fasta, dense_sequences())
    lengths = [c[1] for c in CONTIGS]
    placed_ref = _marked_reference(fasta, None, positions)
    out = {}

    def case(name, ref, setter, reads, seed, tail, lens=lengths):
        table, qual = make_table(reads, lens, seed)
        out[name] = Case(name, ref, setter, table, qual, tail)

    case('placed', placed_ref, 'masks', placed_reads(), 7001, C_LONG)
    case('irregular', placed_ref, 'masks', placed_reads(irregular=True), 7001, C_LONG)
    case('A', placed_ref, 'masks', twin_reads('A'), 7002, -1)
    case('A irregular', placed_ref, 'masks', twin_reads('A') + [Read(C_TWIN1, 10, 50, 0, back_at=30)], 7002, -1)
    case('B', placed_ref, 'masks', twin_reads('B'), 7003, -1)
    case('small', placed_ref, 'masks', [Read(C_LONG, 50, 80, 0), Read(C_LONG, 20, 80, 1), Read(C_LONG, 60, 70, 0)], 7004, -1)
    # one record at most: that of the window the table's last row leaves open
    case('tail only', placed_ref, 'masks', [whole(C_EMPTY, rev, lengths[C_EMPTY]) for rev in (0, 1) * 4] + [Read(C_LONG, 385, 395, 1)],
         7008, C_LONG)
    case('motif', _marked_reference(fasta, MOTIF, None), 'motif', interior_reads(), 7005, C_LEN31)
    case('iupac', _marked_reference(fasta, refmark.parse_motifs(IUPAC, 'A'), None), 'iupac', edge_to_edge_reads(), 7006, C_LONG)
    case('dense', _marked_reference(dense_fasta, 'A', None), 'masks', dense_reads(), 7007, 0, lens=[n for _, n in DENSE_CONTIGS])
    # tables A and B: reducing A's records against B's table must move a count and the number of cross-contig records
    a, b = out['A'], out['B']
    assert b.table.n_seg >= out['A irregular'].table.n_seg > a.table.n_seg and b.table.n_rows > out['A irregular'].table.n_rows
    right, wrong = a.expected(), a.expected(table=b.table)
    assert right.unmarked == 0 and wrong.unmarked == 0, 'a record of table A names no marked site on table B'
    assert right.n_cross != wrong.n_cross and (right.n_total != wrong.n_total).any(), 'table B reduces the records of table A like table A'
    return out


# The named placements of the hand-placed case: (name, contig, strand, position, mask bit of the contig, within k of an end).
# tests/test_site_cases.py finds each as a marked site with records of the oracle.
PLACEMENTS = (
    ('bit 31', C_LONG, 1, 31, 31, False), ('bit 32', C_LONG, 1, 32, 32, False),
    ('bit 63', C_LONG, 0, 63, 63, False), ('bit 64', C_LONG, 1, 64, 64, False),
    ('bit 31 of 64 bases', C_LEN64, 0, 31, 31, False), ('bit 32 of 64 bases', C_LEN64, 1, 32, 32, False),
    ('bit 31 of 65 bases', C_LEN65, 0, 31, 31, False), ('bit 32 of 65 bases', C_LEN65, 1, 32, 32, False),
    ('L - k of 31 bases', C_LEN31, 0, 25, 25, False), ('L - k of 32 bases', C_LEN32, 1, 26, 26, False),
    ('L - k of 33 bases', C_LEN33, 0, 27, 27, False), ('L - k of 64 bases', C_LEN64, 0, 58, 58, False),
    ('L - k of 65 bases', C_LEN65, 1, 59, 59, False), ('L - k of 400 bases', C_LONG, 1, 394, 394, False),
    ('k - 1, the first scoreable position', C_LEN31, 0, 5, 5, False),
    ('k - 2, within k of the start', C_LEN31, 1, 4, 4, True), ('L - k + 1 of 31 bases, within k of the end', C_LEN31, 1, 26, 26, True),
    ('k - 2 of 32 bases', C_LEN32, 0, 4, 4, True), ('L - k + 1 of 32 bases', C_LEN32, 0, 27, 27, True),
    ('L - k + 1 of 64 bases, the last site of its contig', C_LEN64, 1, 59, 59, True),
    ('L - k + 1 of 65 bases', C_LEN65, 0, 60, 60, True), ('k - 2 of 65 bases', C_LEN65, 1, 4, 4, True),
)
# bit 0: position 0 is marked and numbered -- every later site of its strand has one more site before it --, but the window
# machine takes a site at 0 for "no site": it has no record
UNFLUSHED = ((C_LEN33, 0, 0),)
# (last site of a contig, first site of the next contig that has one): neighbours in the numbering, both counted
SEAMS = (((C_LEN64, 1, 59), (C_LEN65, 0, 5)), ((C_LEN65, 1, 59), (C_LONG, 0, 63)))
NAMED_CROSS = (C_LEN64, 0, 58, 'empty')       # (site, the contig its closing row lies on)
