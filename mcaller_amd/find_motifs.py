"""Find methylated motifs de novo from called sites: which short sequence patterns around the called base are mostly methylated?

    python -m mcaller_amd.find_motifs -r ref.fasta --bed SUMMARY.bed [--control CONTROL.bed] [-b A] [--shapes LIST]
                                      [--min_sites 20] [--min_fraction 0.5] [--all] [--iupac] [-o OUT] [--device]
                                      [--iterative [--max_motifs 16] [--unexplained OUT]]

The reference has no such program: its GFF output and `make_bed --control` are shaped for an external motif finder.  This module
closes the loop: every row it prints is a motif in the syntax `--motifs` parses (refmark.parse_motifs).

Inputs.  -r is read with refmark.read_fasta and upper-cased; of several records with one id the last counts.  --bed is a make_bed
summary (plain, --vo or -p form), --control a `make_bed --control` summary.  Of each line only fields 1, 2 and 6 are used: chrom,
0-based start (the index into the contig), strand.  A line with fewer than 6 tab-separated fields, a start int() does not take, a
strand other than + / -, an unknown chrom or a start outside its contig is a ValueError.  A site listed twice counts once.

A CANDIDATE is a (position p, strand) whose base on that strand is --base (on '-': seq[p] is its complement).  It is METHYLATED
if --bed lists it and COVERED if --bed or --control lists it; without --control every candidate is covered.  A listed site whose
reference base is not --base is ignored and counted (n_off_base).

A SHAPE is a string of X and '.', first and last X, at most 24 wide, 2 to 8 X.  For a shape of width W, its j-th X at offset o and
a candidate at p the window is seq[p-o : p-o+W] on '+' and revcomp(seq[p-(W-1-o) : p+o+1]) on '-'.  It counts only if it lies
inside the contig and every letter under an X is one of ACGT; letters under '.' are free.  A counting window adds 1 to
nGenome[shape, j, letters], 1 to nCovered if the candidate is covered and 1 to nMethylated if it is methylated.

A row is SELECTED when nMethylated >= min_sites and float64(nMethylated) / float64(nCovered) >= min_fraction.  Without --all a
selected row is dropped when another selected row (of any shape) has X positions, taken relative to the called base, that are a
strict subset of this row's, with the same letters there: once GATC:2 is selected, GATCA:2 and GATC.....ACG:2 are dropped.

One line per row: SPEC, nGenome, nCovered, nMethylated, fraction, tab-separated.  SPEC is the window with N under every '.',
':' and the 1-based index of the called letter; fraction is repr(float) of the quotient.  Rows are ordered by nMethylated
descending (sites explained, not fraction: a 5-of-5 noise window does not beat GATC at 423 of 423), then fraction descending, then
shape index, j and the letters.

--iupac merges rows into degenerate motifs: GANTC is one row, not its four 5-mers, each of which may miss --min_sites alone.
Per table (shape, j), from the same three counters:
  GOOD      a concrete entry with nCovered >= 1 and float64(nMethylated) / float64(nCovered) >= min_fraction.  An entry that was
            never seen covered vouches for nothing and is not good.
  PATTERN   the called X holds --base, every other X a non-empty subset of ACGT: one of the 15 IUPAC letters
            A C G T R Y S W K M B D H V N, coded as the bit mask A = 1, C = 2, G = 4, T = 8.  Its MEMBERS are the concrete entries
            of the product of its sets, its counts the integer sums of its members' counts.
  PURE      every member is good.  (A sub-pattern of a pure pattern is pure.)
  MAXIMAL   pure, and no pattern made by adding one letter to one X's set is pure -- by the closure above: no strictly larger
            pattern is pure.
A row is a maximal pure pattern with summed nMethylated >= min_sites and float64(nMethylated) / float64(nCovered) >= min_fraction
(the division stays: the mediant of the members' fractions is not trusted to survive rounding).  Without --all a row is dropped when,
for some table whose X positions relative to the called base are a strict subset of this table's, the row's pattern restricted to
those positions is pure in that table -- that table then has a row which covers every occurrence of this one: GATCN:2 of XXXXX is
dropped for GATC:2, GANTC:2 is not, because GANT is not pure.  The line is as above, SPEC with the IUPAC letter of each X's set and
N under every '.'; the order is nMethylated descending, fraction descending, shape index, j, then the masks of the X from left to
right as integers.  Every concrete row of the plain mode is a pure singleton and so contained in some row of --iupac (before the
redundancy rule): the option loses nothing.  `last_counts` gains n_good, n_pure and n_maximal, summed over the tables; n_selected
counts the rows before the redundancy rule.  The host statement builds a table's lattice only inside the box of the letters that
occur, per X, among its good entries (every pure pattern lies in it), not all 15^(k-1) patterns.

--iterative [--max_motifs N] peels the motifs off one at a time; N is 1 to 64, 16 by default, anything else a ValueError.  Round
r = 1, 2, ...:
  1. the report is made exactly as a call without --iterative makes it with the same --shapes, -b, --min_sites, --min_fraction,
     --all and --iupac, but the candidates explained in earlier rounds are NOT CANDIDATES: they add nothing to nGenome, nCovered
     or nMethylated of any table;
  2. a report without a row ends the run;
  3. otherwise its FIRST row, in the order above, is printed with that round's counts (the line format is unchanged: every line is
     a --motifs spec and four numbers);
  4. the row belongs to a table (shape, j) and gives every X of it a set of letters -- a singleton, with --iupac the IUPAC set.  It
     EXPLAINS every remaining candidate (p, strand) whose window in that table counts (inside the contig, every letter under an
     X one of ACGT) and whose letter under X i lies in set i, for every X.  Letters under '.' are free, an N of the reference
     included.  The sets decide, not the SPEC text: in GANNCN:2 of XX..XX the last N is {A, C, G, T}, the middle two are free;
  5. N rows end the run.
The explained candidates of a round are exactly the ones that round's row counted, their number is the row's nGenome; every
printed row explains at least one candidate (nGenome >= nMethylated >= 1 for a row to pass: 0 / 0 is no fraction), so the loop
ends even without --max_motifs; `--iterative --max_motifs 1` prints the first line of the plain call.  `last_counts` holds the
figures of round 1 and gains n_rounds (the rows printed), n_explained (a list: one nGenome per row) and n_unexplained (the
methylated candidates left after the last round: round 1's methylated candidates less the sum of the rows' nMethylated).
--unexplained OUT (only with --iterative) writes those as `chrom\tstart\tstart+1\t.\t.\tstrand\n`, contigs in the reference's
order, start ascending (no base is a candidate of both strands: a total order); the file is a valid --bed for another run.

Out of scope: circular contigs.

`find_motifs` is that definition in NumPy (the host statement; no SciPy, no GPU).  `find_motifs_device` (--device) has the GPU make
the same bytes (Device.motif_report: csrc/motifs/mc_motifscan.hip, --iupac: csrc/motifs/mc_motifiupac.inc, --iterative:
csrc/motifs/mc_motifiter.inc) and runs the host
statement whenever the device declines; `last_report` says who made the output, `last_counts` what the host statement counted."""
import os
import sys

import numpy as np

from . import refmark

last_report = None         # what the last call did: dict(by='device' | 'host', reason=None | str, n_rows=int)
last_counts = None         # the host statement's figures: dict(n_candidates, n_sites, n_control, n_off_base, n_selected)
                           # and, with iupac, n_good, n_pure, n_maximal; with iterative, n_rounds, n_explained, n_unexplained

MAX_WIDTH = 24
MAX_SHAPES = 64            # what the device takes in one call (the host statement has no limit)
MAX_MOTIFS = 64            # --max_motifs: 1 to this
DEFAULT_SHAPES = ['XXX', 'XXXX', 'XXXXX', 'XXXXXX'] + ['X' * a + '.' * g + 'X' * b for a in (3, 4) for g in (5, 6, 7, 8) for b in (3, 4)]
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b'ACGT'):
    _CODE[_c] = _i


def parse_shapes(text):
    """`SHAPE[,SHAPE...]` -> the list; ValueError for anything that is no shape, and for a shape given twice."""
    shapes = [s.strip() for s in text.split(',')] if isinstance(text, str) else list(text)
    for s in shapes:
        if not s or set(s) - set('X.') or s[0] != 'X' or s[-1] != 'X' or len(s) > MAX_WIDTH or not 2 <= s.count('X') <= 8:
            raise ValueError("--shapes entry %r: a shape is a string of X and '.', first and last X, at most %d wide, 2 to 8 X" % (s, MAX_WIDTH))
    if len(set(shapes)) != len(shapes):
        raise ValueError('--shapes %r: a shape is given twice' % (text,))
    return shapes


def read_reference(path):
    """{id: upper-cased sequence}, in file order; of several records with one id the last counts."""
    ref = {}
    for name, seq in refmark.read_fasta(path):
        ref[name] = seq.upper()
    return ref


def read_sites(path, ref):
    """{contig: (bool[len] listed on '+', bool[len] listed on '-')} of a BED file's fields 1, 2 and 6."""
    with open(path, 'rb') as fh:
        lines = fh.read().decode('latin-1').split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    listed = {name: (np.zeros(len(seq), dtype=bool), np.zeros(len(seq), dtype=bool)) for name, seq in ref.items()}
    for n, line in enumerate(lines, 1):
        fields = line.split('\t')
        if len(fields) < 6:
            raise ValueError('%s line %d: %d tab-separated fields, at least 6 are needed' % (path, n, len(fields)))
        start = int(fields[1])
        if fields[5] not in ('+', '-'):
            raise ValueError('%s line %d: strand %r is neither + nor -' % (path, n, fields[5]))
        if fields[0] not in listed:
            raise ValueError('%s line %d: contig %r is not in the reference' % (path, n, fields[0]))
        if not 0 <= start < len(ref[fields[0]]):
            raise ValueError('%s line %d: start %d lies outside contig %r of %d bases' % (path, n, start, fields[0], len(ref[fields[0]])))
        listed[fields[0]][fields[5] == '-'][start] = True
    return listed


def _on_strand(fwd, rev):
    """The letter codes of a contig as its strand reads them: the '-' strand is the '+' strand of the reverse complement, position
    p stands at L - 1 - p there."""
    return np.where(fwd < 4, 3 - fwd, 4).astype(np.uint8)[::-1] if rev else fwd


def count_tables(ref, shapes, base, meth, control, explained=None):
    """-> ([shape][j] -> (nGenome, nCovered, nMethylated), int64 arrays over the 4^k letter codes, first letter highest), counts.
    explained: {contig: (bool[len] '+', bool[len] '-')}, candidates that are none any more (--iterative); the counts do not see it."""
    b = 'ACGT'.index(base)
    tables = [[tuple(np.zeros(4 ** s.count('X'), dtype=np.int64) for _ in range(3)) for _ in range(s.count('X'))] for s in shapes]
    counts = dict(n_candidates=0, n_sites=0, n_control=0, n_off_base=0)
    for name, seq in ref.items():
        fwd = _CODE[np.frombuffer(seq.encode('latin-1', 'replace'), dtype=np.uint8)]
        L = len(fwd)
        for rev in (False, True):
            code = _on_strand(fwd, rev)
            m = meth[name][rev][::-1] if rev else meth[name][rev]
            c = None if control is None else (control[name][rev][::-1] if rev else control[name][rev])
            cand = code == b
            listed = m if c is None else (m | c)
            counts['n_candidates'] += int(cand.sum())
            counts['n_sites'] += int(m.sum())
            counts['n_control'] += 0 if c is None else int(c.sum())
            counts['n_off_base'] += int((listed & ~cand).sum())
            if explained is not None:
                cand = cand & ~(explained[name][rev][::-1] if rev else explained[name][rev])
            is_meth = m & cand
            is_cov = cand if c is None else (listed & cand)
            for si, shape in enumerate(shapes):
                W = len(shape)
                xs = [i for i, ch in enumerate(shape) if ch == 'X']
                n_win = L - W + 1
                if n_win <= 0:
                    continue
                key = np.zeros(n_win, dtype=np.int64)
                ok = np.ones(n_win, dtype=bool)
                for x in xs:
                    piece = code[x:x + n_win]
                    key = key * 4 + (piece & 3)
                    ok &= piece < 4
                for j, o in enumerate(xs):
                    at = ok & cand[o:o + n_win]                # windows whose j-th X is a candidate
                    nG, nC, nM = tables[si][j]
                    size = len(nG)
                    nG += np.bincount(key[at], minlength=size)
                    nC += np.bincount(key[at & is_cov[o:o + n_win]], minlength=size)
                    nM += np.bincount(key[at & is_meth[o:o + n_win]], minlength=size)
    return tables, counts


def _letters(code, k):
    return ''.join('ACGT'[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def report_rows(ref, shapes, base, meth, control, min_sites=20, min_fraction=0.5, keep_all=False, iupac=False, explained=None,
                with_first=False):
    """The rows of the definition as bytes, their number, and the counts.  explained: as in count_tables.  with_first: a fourth
    value, the first row's (shape index, j, the sets of its X from left to right as masks over A = 1, C = 2, G = 4, T = 8), None
    where there is no row."""
    tables, counts = count_tables(ref, shapes, base, meth, control, explained)
    data, n_rows, counts, first = (_iupac_rows if iupac else _plain_rows)(tables, counts, shapes, base, min_sites, min_fraction, keep_all)
    return (data, n_rows, counts, first) if with_first else (data, n_rows, counts)


def _plain_rows(tables, counts, shapes, base, min_sites, min_fraction, keep_all):
    selected = []            # (nM, fraction, shape index, j, letters, nG, nC)
    for si, shape in enumerate(shapes):
        k = shape.count('X')
        for j in range(k):
            nG, nC, nM = tables[si][j]
            with np.errstate(all='ignore'):
                frac = nM.astype(np.float64) / nC.astype(np.float64)
                pick = np.nonzero((nM >= min_sites) & (frac >= np.float64(min_fraction)))[0]
            for code in pick.tolist():
                selected.append((int(nM[code]), float(frac[code]), si, j, _letters(code, k), int(nG[code]), int(nC[code])))
    counts['n_selected'] = len(selected)
    offsets = [[i for i, ch in enumerate(s) if ch == 'X'] for s in shapes]

    def placed(row):         # the row's letters by their place relative to the called base
        xs = offsets[row[2]]
        return frozenset((x - xs[row[3]], ch) for x, ch in zip(xs, row[4]))
    if not keep_all:
        sets = [placed(r) for r in selected]
        have = set(sets)
        kept = []
        for r, mine in zip(selected, sets):
            items = sorted(mine)
            called = [it for it in items if it[0] == 0]
            rest = [it for it in items if it[0] != 0]
            # every strict subset that holds the called base (a row's set always does)
            redundant = any(frozenset(called + [rest[i] for i in range(len(rest)) if sub >> i & 1]) in have for sub in range(2 ** len(rest) - 1))
            if not redundant:
                kept.append(r)
        selected = kept
    selected.sort(key=lambda r: (-r[0], -r[1], r[2], r[3], r[4]))
    out = []
    for nM, frac, si, j, letters, nG, nC in selected:
        window, it = [], iter(letters)
        for ch in shapes[si]:
            window.append(next(it) if ch == 'X' else 'N')
        out.append('%s:%d\t%d\t%d\t%d\t%s\n' % (''.join(window), offsets[si][j] + 1, nG, nC, nM, repr(frac)))
    first = (selected[0][2], selected[0][3], tuple(1 << 'ACGT'.index(ch) for ch in selected[0][4])) if selected else None
    return ''.join(out).encode('ascii'), len(out), counts, first


IUPAC_LETTER = ' ACMGRSVTWYHKDBN'            # the letter of a set over A = 1, C = 2, G = 4, T = 8


def _lattice(good):
    """good: bool [4] * n over the letters of the free X -> (box, pure, maximal) or None where nothing is good.  box[i]: the letter
    codes that occur at free X i among the good entries, ascending; pure and maximal: bool [2 ** len(box[i]) - 1 for i], index
    s - 1 at X i is the set of box[i][l] for the bits l of s.  Every pure pattern lies in the box, so nothing outside is built."""
    n = good.ndim
    box = [np.nonzero(good.any(axis=tuple(a for a in range(n) if a != i)))[0] for i in range(n)]
    if not len(box[0]):
        return None
    pure = good[np.ix_(*box)]
    for i in range(n):                           # the AND transform, one X at a time: 4 letters -> their non-empty sets
        b = len(box[i])
        pure = np.stack([np.logical_and.reduce(pure.take([l for l in range(b) if sub >> l & 1], axis=i), axis=i) for sub in range(1, 2 ** b)], axis=i)
    maximal = pure.copy()
    for i in range(n):                           # (a letter from outside the box never keeps a pattern pure)
        subs = np.arange(1, 2 ** len(box[i]))
        along = [1] * n
        along[i] = -1
        for l in range(len(box[i])):
            grown = subs | (1 << l)
            maximal &= ~(pure.take(grown - 1, axis=i) & (grown != subs).reshape(along))
    return box, pure, maximal


def _iupac_rows(tables, counts, shapes, base, min_sites, min_fraction, keep_all):
    """report_rows for --iupac: the maximal pure patterns of every table over both thresholds, less those a smaller table explains."""
    b = 'ACGT'.index(base)
    offsets = [[i for i, ch in enumerate(s) if ch == 'X'] for s in shapes]
    lattices = {}                                # (shape index, j) -> _lattice of the table
    selected = []                                # (nM, fraction, shape index, j, masks of the X, nG, nC)
    counts.update(n_good=0, n_pure=0, n_maximal=0)
    for si, shape in enumerate(shapes):
        k = shape.count('X')
        for j in range(k):
            nG, nC, nM = (a.reshape((4,) * k).take(b, axis=j) for a in tables[si][j])
            with np.errstate(all='ignore'):
                good = (nC >= 1) & (nM.astype(np.float64) / nC.astype(np.float64) >= np.float64(min_fraction))
            counts['n_good'] += int(good.sum())
            lat = lattices[si, j] = _lattice(good)
            if lat is None:
                continue
            box, pure, maximal = lat
            counts['n_pure'] += int(pure.sum())
            counts['n_maximal'] += int(maximal.sum())
            for at in np.argwhere(maximal).tolist():
                members = [[int(box[i][l]) for l in range(len(box[i])) if (s + 1) >> l & 1] for i, s in enumerate(at)]
                cells = np.ix_(*members)
                sums = [int(a[cells].sum()) for a in (nG, nC, nM)]
                frac = np.float64(sums[2]) / np.float64(sums[1])         # (a pure pattern's members are covered: no 0 / 0)
                if sums[2] >= min_sites and frac >= np.float64(min_fraction):
                    masks = [sum(1 << c for c in m) for m in members]
                    masks.insert(j, 1 << b)
                    selected.append((sums[2], float(frac), si, j, tuple(masks), sums[0], sums[1]))
    counts['n_selected'] = len(selected)

    def is_pure(si, j, masks):                   # masks of the free X of table (si, j)
        lat = lattices[si, j]
        if lat is None:
            return False
        at = []
        for letters, mask in zip(lat[0], masks):
            local = sum(1 << l for l, c in enumerate(letters.tolist()) if mask >> c & 1)
            if local == 0 or (sum(1 << c for c in letters.tolist()) & mask) != mask:       # a letter from outside the box
                return False
            at.append(local - 1)
        return bool(lat[1][tuple(at)])
    if not keep_all:
        kept = []
        for row in selected:
            si, j, masks = row[2], row[3], row[4]
            mine = {x - offsets[si][j]: m for x, m in zip(offsets[si], masks)}
            redundant = False
            for ui in range(len(shapes)):
                for uj in range(len(offsets[ui])):
                    theirs = [x - offsets[ui][uj] for x in offsets[ui]]
                    if len(theirs) < len(mine) and all(r in mine for r in theirs):
                        redundant = redundant or is_pure(ui, uj, [mine[r] for r in theirs if r != 0])
            if not redundant:
                kept.append(row)
        selected = kept
    selected.sort(key=lambda r: (-r[0], -r[1], r[2], r[3], r[4]))
    out = []
    for nM, frac, si, j, masks, nG, nC in selected:
        window, it = [], iter(masks)
        for ch in shapes[si]:
            window.append(IUPAC_LETTER[next(it)] if ch == 'X' else 'N')
        out.append('%s:%d\t%d\t%d\t%d\t%s\n' % (''.join(window), offsets[si][j] + 1, nG, nC, nM, repr(frac)))
    first = (selected[0][2], selected[0][3], tuple(selected[0][4])) if selected else None
    return ''.join(out).encode('ascii'), len(out), counts, first


def explain(ref, shapes, base, first, explained):
    """Step 4 of --iterative: marks in `explained` every remaining candidate the row `first` (shape index, j, masks) explains ->
    their number."""
    b = 'ACGT'.index(base)
    si, j, masks = first
    xs = [i for i, ch in enumerate(shapes[si]) if ch == 'X']
    W, o = len(shapes[si]), xs[j]
    member = [np.array([m >> c & 1 for c in range(4)] + [0], dtype=bool) for m in masks]      # code 4 (no ACGT) is in no set
    n = 0
    for name, seq in ref.items():
        fwd = _CODE[np.frombuffer(seq.encode('latin-1', 'replace'), dtype=np.uint8)]
        n_win = len(fwd) - W + 1
        if n_win <= 0:
            continue
        for rev in (False, True):
            code = _on_strand(fwd, rev)
            mine = explained[name][rev][::-1] if rev else explained[name][rev]                 # a view: position p at L - 1 - p
            hit = (code[o:o + n_win] == b) & ~mine[o:o + n_win]
            for x, inside in zip(xs, member):
                hit &= inside[code[x:x + n_win]]
            mine[o:o + n_win] |= hit
            n += int(hit.sum())
    return n


def iterative_rows(ref, shapes, base, meth, control, min_sites=20, min_fraction=0.5, keep_all=False, iupac=False, max_motifs=16):
    """--iterative: the first row of every round as bytes, their number, the counts of round 1 with n_rounds, n_explained and
    n_unexplained, and the left-over sites as the --unexplained bytes."""
    explained = {name: (np.zeros(len(seq), dtype=bool), np.zeros(len(seq), dtype=bool)) for name, seq in ref.items()}
    out, n_explained, counts = [], [], None
    while len(out) < max_motifs:
        data, n_rows, now, first = report_rows(ref, shapes, base, meth, control, min_sites, min_fraction, keep_all, iupac, explained, True)
        counts = counts or now
        if n_rows == 0:
            break
        out.append(data[:data.index(b'\n') + 1])
        n_explained.append(explain(ref, shapes, base, first, explained))
        if n_explained[-1] != int(out[-1].split(b'\t')[1]):
            raise AssertionError('the row %r explains %d candidates' % (out[-1], n_explained[-1]))
    b = 'ACGT'.index(base)
    left = []
    for name, seq in ref.items():
        fwd = _CODE[np.frombuffer(seq.encode('latin-1', 'replace'), dtype=np.uint8)]
        plus = meth[name][0] & (fwd == b) & ~explained[name][0]
        minus = meth[name][1] & (fwd == 3 - b) & ~explained[name][1]
        at = np.nonzero(plus | minus)[0]
        left += ['%s\t%d\t%d\t.\t.\t%s\n' % (name, p, p + 1, '-' if minus[p] else '+') for p in at.tolist()]
    counts.update(n_rounds=len(out), n_explained=n_explained, n_unexplained=len(left))
    return b''.join(out), len(out), counts, ''.join(left).encode('latin-1', 'replace')


def _write(out, data):
    """data (bytes) to `out`: None is stdout, a str a path, anything else a file object."""
    if isinstance(out, (str, os.PathLike)):
        with open(out, 'wb') as fo:
            fo.write(data)
        return
    fo = sys.stdout if out is None else out
    if hasattr(fo, 'buffer'):
        fo.flush()
        fo.buffer.write(data)
        fo.buffer.flush()
    else:
        try:
            fo.write(data.decode('ascii'))
        except TypeError:
            fo.write(data)


def _checked(base, shapes, min_sites, min_fraction):
    base = str(base).upper()
    if base not in ('A', 'C', 'G', 'T'):
        raise ValueError('--base %r: the called base is one of A, C, G, T' % base)
    shapes = parse_shapes(DEFAULT_SHAPES if shapes is None else shapes)
    min_sites = int(min_sites)
    min_fraction = float(min_fraction)
    if min_sites < 0 or not min_fraction >= 0.0:
        raise ValueError('--min_sites and --min_fraction are not negative')
    return base, shapes, min_sites, min_fraction


def _checked_iterative(iterative, max_motifs, unexplained):
    if unexplained is not None and not iterative:
        raise ValueError('--unexplained goes with --iterative')
    if isinstance(max_motifs, bool) or not isinstance(max_motifs, (int, np.integer)) or not 1 <= max_motifs <= MAX_MOTIFS:
        raise ValueError('--max_motifs %r: 1 to %d' % (max_motifs, MAX_MOTIFS))
    return int(max_motifs)


def _host(reference, bed, control, base, shapes, min_sites, min_fraction, keep_all, out, reason, iupac=False, iterative=False, max_motifs=16,
          unexplained=None):
    global last_report, last_counts
    last_report = last_counts = None
    ref = read_reference(reference)
    meth = read_sites(bed, ref)
    ctl = None if control is None else read_sites(control, ref)
    if iterative:
        data, n_rows, counts, left = iterative_rows(ref, shapes, base, meth, ctl, min_sites, min_fraction, keep_all, iupac, max_motifs)
        if unexplained is not None:
            _write(unexplained, left)
    else:
        data, n_rows, counts = report_rows(ref, shapes, base, meth, ctl, min_sites, min_fraction, keep_all, iupac)
    _write(out, data)
    last_counts = counts
    last_report = dict(by='host', reason=reason, n_rows=n_rows)
    return n_rows


def find_motifs(reference, bed, control=None, base='A', shapes=None, min_sites=20, min_fraction=0.5, keep_all=False, out=None, iupac=False,
                iterative=False, max_motifs=16, unexplained=None):
    """The host statement: the definition above in NumPy -> the number of rows."""
    base, shapes, min_sites, min_fraction = _checked(base, shapes, min_sites, min_fraction)
    max_motifs = _checked_iterative(iterative, max_motifs, unexplained)
    return _host(reference, bed, control, base, shapes, min_sites, min_fraction, keep_all, out, 'the host statement was asked for', iupac,
                 iterative, max_motifs, unexplained)


def find_motifs_device(reference, bed, control=None, base='A', shapes=None, min_sites=20, min_fraction=0.5, keep_all=False, out=None,
                        iupac=False, iterative=False, max_motifs=16, unexplained=None):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_report, last_counts
    base, shapes, min_sites, min_fraction = _checked(base, shapes, min_sites, min_fraction)
    max_motifs = _checked_iterative(iterative, max_motifs, unexplained)
    last_report = last_counts = None
    if len(shapes) > MAX_SHAPES:
        reason = 'the device takes at most %d shapes in one call' % MAX_SHAPES
    else:
        from .device import get_device
        ref = read_reference(reference)
        if iterative:
            blob, n_rows, reason, left = get_device().motif_report(ref, path=bed, control_path=control, base=base, shapes=shapes,
                                                                   min_sites=min_sites, min_fraction=min_fraction, keep_all=keep_all,
                                                                   iupac=iupac, iterative=True, max_motifs=max_motifs,
                                                                   left=unexplained is not None)
        else:
            blob, n_rows, reason = get_device().motif_report(ref, path=bed, control_path=control, base=base, shapes=shapes, min_sites=min_sites,
                                                             min_fraction=min_fraction, keep_all=keep_all, iupac=iupac)
        if blob is not None:
            if unexplained is not None:
                _write(unexplained, left)
            _write(out, blob)
            last_report = dict(by='device', reason=None, n_rows=n_rows)
            return n_rows
    return _host(reference, bed, control, base, shapes, min_sites, min_fraction, keep_all, out, reason, iupac, iterative, max_motifs, unexplained)


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Report the sequence patterns around the called base whose occurrences are mostly methylated')
    parser.add_argument('-r', '--reference', type=str, required=True, help='fasta file with the reference the sites were called on')
    parser.add_argument('--bed', type=str, required=True, help='summary bed file from make_bed (plain, --vo or -p): the methylated sites')
    parser.add_argument('--control', type=str, required=False, help='summary from make_bed --control: covered sites that were not called')
    parser.add_argument('-b', '--base', type=str, required=False, default='A', help='the called base (default: A)')
    parser.add_argument('--shapes', type=str, required=False,
                        help="comma list of shapes of X and '.' (default: XXX to XXXXXX and the bipartite X{3,4}.{5-8}X{3,4})")
    parser.add_argument('--min_sites', type=int, required=False, default=20, help='methylated occurrences a row needs (default: 20)')
    parser.add_argument('--min_fraction', type=float, required=False, default=0.5,
                        help='methylated / covered occurrences a row needs (default: 0.5)')
    parser.add_argument('--all', action='store_true', required=False, help='keep rows that a shorter selected row explains')
    parser.add_argument('--iupac', action='store_true', required=False, help='merge rows into degenerate (IUPAC) motifs')
    parser.add_argument('-o', '--output', type=str, required=False, help='write the rows to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', required=False, help='count on the GPU (the host statement runs when it declines)')
    parser.add_argument('--iterative', action='store_true', required=False,
                        help='print the best row, set the candidates it explains aside, look again; until nothing passes')
    parser.add_argument('--max_motifs', type=int, required=False, default=16, help='with --iterative: at most this many rows, 1 to 64 (default: 16)')
    parser.add_argument('--unexplained', type=str, required=False,
                        help='with --iterative: write the methylated sites no printed row explains to this file, as a bed')
    args = parser.parse_args(argv)
    if args.unexplained is not None and not args.iterative:
        parser.error('--unexplained goes with --iterative')

    assert os.path.isfile(args.reference), 'file not found at ' + args.reference
    assert os.path.isfile(args.bed), 'file not found at ' + args.bed
    assert args.control is None or os.path.isfile(args.control), 'file not found at ' + args.control

    run = find_motifs_device if args.device else find_motifs
    return run(args.reference, args.bed, args.control, args.base, args.shapes, args.min_sites, args.min_fraction, args.all, args.output,
               args.iupac, args.iterative, args.max_motifs, args.unexplained)


if __name__ == '__main__':
    main()
