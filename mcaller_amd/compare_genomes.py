"""Compare two `make_bed --vo` BED files site by site: do the two samples' per-read methylation probabilities differ?

    python -m mcaller_amd.compare_genomes --bed1 A.bed --bed2 B.bed [-g XMFA] [-o OUT] [--device] [-v]

The reference's program of this name (compare_genomes.py) reads the two files into dictionaries keyed by (chrom, start, end,
strand) and runs four SciPy tests per shared key.  UNLIKE THE REFERENCE, sample 1 is tested against sample 2 here:
compare_genomes.py:21-29 passes bed1's probabilities as both arguments of every test, so ks_2samp(x, x) has p = 1, the
`pval4 < 0.9` filter lets nothing through and the program prints nothing for any input.  There is no p-value filter here either:
every shared key gets a row.

One row per key of bed1 that bed2 also has, in bed1's file order, tab-separated:

    chrom start end strand frac1 depth1 frac2 depth2 U z_mwu z_rs t D nlp_mwu nlp_rs nlp_t nlp_ks

frac and depth are fields 5 and 7 of the two lines as they stand; x and y are the probability lists (field 8) of the key's
line in bed1 and bed2.  U, z_mwu, nlp_mwu: mannwhitneyu(x, y, alternative='two-sided', method='asymptotic') (U of x; z is
SciPy's standardized statistic with tie and continuity correction); z_rs, nlp_rs: ranksums(x, y); t, nlp_t: ttest_ind(x, y);
D: ks_2samp's statistic, nlp_ks from Smirnov's limit kstwobign.sf(sqrt(n1 n2 / (n1 + n2)) D).  U is str(float(U)), D its repr,
z and t are str(np.round(v, 3)), every nlp is str(np.round(0.0 - np.log10(p), 3)).

`compare_by_position` is that definition written with the SciPy calls (the host statement).  `compare_by_position_device`
(--device) has the GPU make the same bytes (Device.bed_compare: csrc/compare/mc_bedcompare.hip) and runs the host statement
whenever the device declines; `last_compare` says who made the output.  -g is accepted and unused, as in the reference.

TWO GENOMES WITH THEIR OWN ASSEMBLIES are compared through a Mauve alignment (the reference declares -g and never reads it):

    python -m mcaller_amd.compare_genomes --bed1 A.bed --bed2 B.bed --xmfa AB.xmfa --fai1 A.fasta.fai --fai2 B.fasta.fai
                                          [--xmfa_seqs 1,2] [-o OUT] [--device]

.fai files: the first two tab-separated fields of each non-blank line, name and length, in file order.  Mauve numbers a
multi-FASTA genome in concatenated coordinates in that order: contig k starts at offset sum(len[:k]).  Of two contigs with one
name the first is meant.

XMFA lines: lines beginning with '#' and empty lines are ignored.  A block is a run of entries ended by a line that is exactly
'='.  An entry is a header line followed by sequence lines of any widths.  The header is '>', optional blanks (spaces, tabs), then
SEQ:START-END, one or more blanks, '+' or '-', and optionally a blank followed by anything; SEQ, START and END are plain decimal,
coordinates 1-based and inclusive in concatenated coordinates.  A sequence byte is '-' (a gap) or an ASCII letter.
Entries: START-END of 0-0 means the sequence is absent from the block: the entry must be all gaps and contributes nothing; any
other entry has 1 <= START <= END and END - START + 1 non-gaps.  All entries of a block have the same number of columns.  The
non-gap of rank r (0-based) of a '+' entry is coordinate START + r, of a '-' entry END - r.
Columns: for the two sequence numbers of --xmfa_seqs (bed1's genome, then bed2's; the block's first entry of each number), a
column where both are non-gap maps g1 -> (g2, flip), flip: the two entries' strands differ.  A block that lacks either sequence
maps nothing.  A g1 aligned more than once keeps the first column in file order.
Lifting a bed1 line (chrom, start, end, strand, ...): chrom is a name of --fai1, start plain digits (no sign, no blanks, no
leading zero unless it is 0; the host takes whatever else int() accepts, and a line whose start int() rejects has no image),
g1 = off1[chrom] + start + 1 <= off1[chrom] + len1[chrom], strand '+' or '-'.  Its image is the bed2 key (chrom2, str(start2),
str(start2 + 1), strand2): g2 falls in contig chrom2 of --fai2, start2 = g2 - off2[chrom2] - 1, strand2 the strand, flipped if
flip.  The image is matched against bed2's (chrom, start, end, strand) as text.  A line with an unknown chrom, a start past its
contig, a strand that is neither '+' nor '-' or an unmapped g1 has no image: it is counted in last_compare['n_unaligned'] (per
key of bed1) and writes no row.
One row per bed1 line whose image is a key of bed2, in bed1's order:

    chrom1 start1 end1 strand1 chrom2 start2 end2 strand2 frac1 depth1 frac2 depth2 U z_mwu z_rs t D nlp_mwu nlp_rs nlp_t nlp_ks

with the nine statistics of the row above for the same two lists.
Errors (ValueError, 'xmfa line N: ...'): line by line, the first offending line and on it the first of: a '\r' or a byte >= 0x80;
a malformed header, or a sequence line before its block's first header; a sequence byte that is neither '-' nor a letter.  In a
file whose lines are sound, entry by entry (the header's line is named), the first of: a non-gap count that disagrees with the
header; a column count other than that of the entry before it in the block; an entry behind the last '='; an END beyond the
.fai total of its genome (--xmfa_seqs' two).  The device declines on each (MC_CMP_DECLINE_XMFA_*) and this statement words the error;
it also declines a bed1 start that is not plain digits, and this statement does the file.

A COUNT TEST AND A MULTIPLE-TESTING CORRECTION:

    python -m mcaller_amd.compare_genomes --bed1 A.bed --bed2 B.bed [--xmfa ... --fai1 ... --fai2 ...] [--fisher] [--fdr] [-o OUT] [--device]

Rows, their order and the first 17 columns (21 with --xmfa) stay as they are; without the flags every byte does.  Appended:

    ... nlp_ks [nlp_fisher] [nlq_mwu nlq_rs nlq_t nlq_ks [nlq_fisher]]

Counts (--fisher only; frac is not parsed without it): for a line, n = len(probabilities), f = float(frac) (field 5) and
K = int(np.rint(f * n)).  The line is sound iff 0 <= K <= n and np.float64(K) / np.float64(n) == f: frac is the str(np.mean(labels))
make_bed wrote (the rule recovers K for every 0 <= K <= n <= 8192).  A shared line that is not sound is
ValueError('bed<i> line <no>: frac is not a count over its reads'); the depth field stays opaque text.
nlp_fisher: X ~ Hypergeometric(N = n1 + n2, K = K1 + K2, d = n1), observed K1; the two-sided p is the sum of P(x) over
{x : P(x) <= P(K1) (1 + 10^-7)}, compared in exact rationals (fractions.Fraction; the factor is R's, the fp64 number).  Printed:
str(np.round(0.0 - L, 3)), L the fp64 number nearest to log10 of the exact rational p (decimal, 60 digits); p = 1 prints 0.0.
nlq_* (Benjamini-Hochberg in the log domain, per column): L_i the unrounded log10 p of row i (np.log10 of SciPy's p for the four
tests, L above for Fisher's), m the rows whose L_i is not NaN, sorted ascending, ranks j = 1 .. m:
    T_(j) = L_(j) + (np.log10(np.float64(m)) - np.log10(np.float64(j)))          Q_(j) = min(0.0, min over k >= j of T_(k))
Tied L get one Q however they are sorted.  Printed: str(np.round(0.0 - Q_i, 3)); a NaN row prints nan and is not counted in m; m
counts the rows written, not bed1's lines.  10 ** Q is scipy.stats.false_discovery_control(p) to 1.4e-15.
On the GPU (--device; csrc/mc_fisher.h, csrc/mc_bh.h, csrc/compare/mc_cmpfdr.inc): the host statement's bytes, or a decline and the
host statement -- a shared line whose frac the device's decimal reader declines or that is no count (this statement words the error),
a Fisher log10 p below -250, a mass within its derived error of the selection factor, a value (nlp_fisher or a q-value) within its
derived bound of a rounding tie, too little device memory for the sort buffers (MC_CMP_DECLINE_*)."""
import functools
import os
import re
import sys
import warnings

import numpy as np

# what the last comparison did: dict(by='device' | 'host', reason=None | str, n_sites=int), and n_unaligned=int with --xmfa
last_compare = None


def read_bed(bed):
    """{(chrom, start, end, strand): ((frac, depth), probabilities)} of a --vo BED file, the reference's loop (compare_genomes.py:
    11-16): a line that does not have 8 fields is its tuple-unpacking ValueError; a later duplicate of a key keeps the first
    position and takes the last value."""
    sites = {}
    with open(bed, 'r') as fi:
        for line in fi:
            csome, start, end, motif, perc_meth, strand, num_reads, probabilities = tuple(line.split('\t'))
            sites[(csome, start, end, strand)] = ((perc_meth, num_reads), np.asarray([float(p) for p in probabilities.strip().split(',')]))
    return sites


def site_values(x, y, logs=None):
    """The nine printed values of a site, as text, from the SciPy calls of the definition; logs (a list): the unrounded log10 p of the
    four tests are appended to it."""
    from scipy.stats import ks_2samp, kstwobign, mannwhitneyu, ranksums, ttest_ind
    n1, n2 = len(x), len(y)
    n = n1 + n2
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        mwu = mannwhitneyu(x, y, alternative='two-sided', method='asymptotic')
        U1 = mwu.statistic
        # SciPy's standardized statistic (_get_mwu_z), which mannwhitneyu does not hand out
        _, counts = np.unique(np.concatenate([x, y]), return_counts=True)
        counts = counts.astype(np.float64)
        tie_term = (counts**3 - counts).sum()
        s = np.sqrt(n1 * n2 / 12 * ((n + 1) - tie_term / (n * (n - 1))))
        numerator = np.maximum(U1, n1 * n2 - U1) - n1 * n2 / 2
        numerator -= 0.5
        z_mwu = np.float64(numerator) / s
        rs = ranksums(x, y)
        tt = ttest_ind(x, y)
        D = ks_2samp(x, y, method='asymp').statistic
        p_ks = kstwobign.sf(np.sqrt(n1 * n2 / (n1 + n2)) * D)
        nlp = [str(np.round(0.0 - np.log10(p), 3)) for p in (mwu.pvalue, rs.pvalue, tt.pvalue, p_ks)]
        if logs is not None:
            logs.extend(np.log10(p) for p in (mwu.pvalue, rs.pvalue, tt.pvalue, p_ks))
        return [str(float(U1)), str(np.round(z_mwu, 3)), str(np.round(rs.statistic, 3)), str(np.round(tt.statistic, 3)),
                repr(float(D))] + nlp


_FISHER_FACTOR = None


def site_counts(frac, n):
    """K of a line with n probabilities whose field 5 is `frac`, the str(np.mean(labels)) make_bed wrote, or None when the
    text is not a count over n reads."""
    try:
        f = float(frac)
    except ValueError:
        return None
    if n < 1 or not np.isfinite(f):
        return None
    K = int(np.rint(f * n))
    if not 0 <= K <= n or np.float64(K) / np.float64(n) != f:
        return None
    return K


def fisher_log10p(K1, n1, K2, n2):
    """The fp64 number nearest to log10 of the two-sided p of Fisher's exact test on K1 of n1 against K2 of n2, in exact rationals:
    X ~ Hypergeometric(n1 + n2, K1 + K2, n1), p the sum of P(x) over the x with P(x) <= P(K1) (1 + 10^-7)."""
    from decimal import Context, Decimal
    from fractions import Fraction
    from math import comb
    global _FISHER_FACTOR
    if _FISHER_FACTOR is None:
        _FISHER_FACTOR = Fraction(1.0 + 1e-7)               # R's factor, the fp64 number itself
    if not (0 <= K1 <= n1 and 0 <= K2 <= n2):
        raise ValueError('fisher_log10p: not 0 <= K1 <= n1, 0 <= K2 <= n2')
    N, K, d = n1 + n2, K1 + K2, n1
    lo, hi = max(0, d - (N - K)), min(K, d)
    mass = [comb(K, lo) * comb(N - K, d - lo)]                               # P(x) C(N, d) = C(K, x) C(N - K, d - x): integers
    for x in range(lo, hi):                                                  # (the ratio of two neighbours, an exact division)
        mass.append(mass[-1] * ((K - x) * (d - x)) // ((x + 1) * (N - K - d + x + 1)))
    limit = mass[K1 - lo] * _FISHER_FACTOR
    part, total = sum(w for w in mass if w <= limit), sum(mass)
    if part == total:
        return 0.0
    ctx = Context(prec=60)
    return float(ctx.log10(ctx.divide(Decimal(part), Decimal(total))))


def fisher_nlp(K1, n1, K2, n2):
    """The printed value of the nlp_fisher column."""
    return str(np.round(0.0 - fisher_log10p(K1, n1, K2, n2), 3))


def bh_log10(L):
    """log10 of the Benjamini-Hochberg q-values of a column of log10 p (float64 [n]; NaN: the row is not tested and stays NaN):
    with the m tested rows sorted ascending, Q_(j) = min(0, min over k >= j of L_(k) + (log10 m - log10 k))."""
    L = np.asarray(L, dtype=np.float64).reshape(-1)
    Q = np.full(len(L), np.nan)
    tested = np.flatnonzero(~np.isnan(L))
    m = len(tested)
    if m == 0:
        return Q
    order = tested[np.argsort(L[tested], kind='stable')]
    T = L[order] + (np.log10(np.float64(m)) - np.log10(np.arange(1, m + 1, dtype=np.float64)))
    Q[order] = np.minimum(0.0, np.minimum.accumulate(T[::-1])[::-1])
    return Q


def _line_numbers(bed):
    """{key: 1-based number of the line whose value read_bed keeps (the last of a key)}"""
    numbers = {}
    with open(bed, 'r') as fi:
        for no, line in enumerate(fi, 1):
            fields = line.split('\t')
            numbers[(fields[0], fields[1], fields[2], fields[5])] = no
    return numbers


class _Extra(object):
    """The columns behind nlp_ks: per row the unrounded log10 p of the four tests and of Fisher's, then the q-values."""

    def __init__(self, bed1, bed2, fisher, fdr):
        self.fisher, self.fdr, self.logs = fisher, fdr, []
        self.numbers = (_line_numbers(bed1), _line_numbers(bed2)) if fisher else None

    def site(self):
        """-> the row's list of logs, for site_values to fill"""
        row = []
        self.logs.append(row)
        return row

    def fisher_column(self, row, key1, key2, site1, site2):
        counts = []
        for which, (key, ((frac, _), p)) in enumerate(((key1, site1), (key2, site2))):
            K = site_counts(frac, len(p))
            if K is None:
                raise ValueError('bed%d line %d: frac is not a count over its reads' % (which + 1, self.numbers[which][key]))
            counts += [K, len(p)]
        L = fisher_log10p(*counts)
        row.append(L)
        return str(np.round(0.0 - L, 3))

    def finish(self, rows):
        """rows: lists of fields; the q-value columns are appended in place"""
        if not self.fdr or not rows:
            return
        with np.errstate(all='ignore'):
            for L in np.asarray(self.logs, dtype=np.float64).T:
                for fields, q in zip(rows, bh_log10(L)):
                    fields.append(str(np.round(0.0 - q, 3)))


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


def read_fai(path):
    """(names, lens int64 [k], offs int64 [k + 1]) of a .fai file: name and length of every non-blank line, in file order;
    offs[k] is the genome's length in concatenated coordinates."""
    names, lens = [], []
    with open(path, 'r') as fi:
        for no, line in enumerate(fi, 1):
            if not line.strip():
                continue
            fields = line.rstrip('\n').split('\t')
            if len(fields) < 2 or not fields[1].isascii() or not fields[1].isdigit():
                raise ValueError('%s line %d: not a name and a length' % (path, no))
            names.append(fields[0])
            lens.append(int(fields[1]))
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens, dtype=np.int64)
    return names, lens, offs


_XMFA_HEADER = re.compile(rb'>[ \t]*([0-9]+):([0-9]+)-([0-9]+)[ \t]+([+-])(?:[ \t].*)?', re.S)
_XMFA_NOT_SEQ = re.compile(rb'[^A-Za-z-]')


def _xmfa_error(no, what):
    return ValueError('xmfa line %d: %s' % (no, what))


def xmfa_blocks(path):
    """The entries of an XMFA file, line-level errors raised: [(closed, [(header's 1-based line, seq, start, end, strand, joined
    sequence bytes)])], one per block in file order; the entries behind the last '=' are a block that is not closed."""
    with open(path, 'rb') as fi:
        lines = fi.read().split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    blocks, cur = [], []
    for no, line in enumerate(lines, 1):
        if b'\r' in line or not line.isascii():
            raise _xmfa_error(no, "a '\\r' or a byte >= 0x80")
        if not line or line[:1] == b'#':
            continue
        if line == b'=':
            blocks.append((True, cur))
            cur = []
        elif line[:1] == b'>':
            m = _XMFA_HEADER.fullmatch(line)
            if m is None:
                raise _xmfa_error(no, 'a malformed header')
            seq, start, end = int(m.group(1)), int(m.group(2)), int(m.group(3))
            if (start, end) != (0, 0) and not 1 <= start <= end:
                raise _xmfa_error(no, 'a malformed header (START-END is neither 0-0 nor 1 <= START <= END)')
            cur.append([no, seq, start, end, m.group(4).decode(), []])
        else:
            if not cur:
                raise _xmfa_error(no, "a sequence line before its block's first header")
            if _XMFA_NOT_SEQ.search(line):
                raise _xmfa_error(no, "a sequence byte that is neither '-' nor a letter")
            cur[-1][5].append(line)
    if cur:
        blocks.append((False, cur))
    return [(closed, [tuple(e[:5]) + (b''.join(e[5]),) for e in entries]) for closed, entries in blocks]


def xmfa_map(path, n1, seqs=(1, 2), n2=None):
    """The coordinate map of the definition for genome seqs[0] (n1 bases) onto genome seqs[1] (n2 bases, None: not checked)
    -> (g2: int64 [n1 + 1], flip: uint8 [n1 + 1]), index g1, 0: unmapped."""
    seq1, seq2 = int(seqs[0]), int(seqs[1])
    if seq1 == seq2:
        raise ValueError('xmfa_map: two different sequence numbers')
    G1, G2, F = [], [], []
    for closed, entries in xmfa_blocks(path):
        pick = {}
        for k, (no, seq, start, end, strand, text) in enumerate(entries):
            cols = len(text)
            if cols - text.count(b'-') != (0 if end == 0 else end - start + 1):
                raise _xmfa_error(no, "a non-gap count that disagrees with the header's %d-%d" % (start, end))
            if k > 0 and cols != len(entries[k - 1][5]):
                raise _xmfa_error(no, 'unequal column counts in a block')
            if not closed:
                raise _xmfa_error(no, "an entry behind the last '=' without a closing '='")
            if (seq == seq1 and end > n1) or (seq == seq2 and n2 is not None and end > n2):
                raise _xmfa_error(no, 'a coordinate beyond the .fai total of its genome')
            pick.setdefault(seq, k)
        if seq1 not in pick or seq2 not in pick:
            continue
        _, _, s1, e1, st1, t1 = entries[pick[seq1]]
        _, _, s2, e2, st2, t2 = entries[pick[seq2]]
        if e1 == 0 or e2 == 0:
            continue
        a1, a2 = np.frombuffer(t1, dtype=np.uint8) != 45, np.frombuffer(t2, dtype=np.uint8) != 45
        both = np.flatnonzero(a1 & a2)
        r1, r2 = np.cumsum(a1, dtype=np.int64)[both] - 1, np.cumsum(a2, dtype=np.int64)[both] - 1
        G1.append(s1 + r1 if st1 == '+' else e1 - r1)
        G2.append(s2 + r2 if st2 == '+' else e2 - r2)
        F.append(np.full(len(both), st1 != st2, dtype=np.uint8))
    g2, flip = np.zeros(n1 + 1, dtype=np.int64), np.zeros(n1 + 1, dtype=np.uint8)
    if G1:
        at, first = np.unique(np.concatenate(G1), return_index=True)          # the first column in file order wins
        g2[at], flip[at] = np.concatenate(G2)[first], np.concatenate(F)[first]
    return g2, flip


def plain_digits(text):
    return text.isascii() and text.isdigit() and (text == '0' or text[0] != '0')


def lift_key(key, contigs1, contigs2, g2, flip):
    """The image of bed1's key (chrom, start, end, strand) in bed2's coordinates, or None.  contigs: ({name: index}, lens, offs,
    names)."""
    chrom, start, _, strand = key
    index1, lens1, offs1, _ = contigs1
    _, _, offs2, names2 = contigs2
    k = index1.get(chrom)
    if k is None or strand not in ('+', '-'):
        return None
    if plain_digits(start):
        start = int(start)
    else:
        try:
            start = int(start)
        except ValueError:
            return None
    if not 0 <= start < lens1[k]:
        return None
    to = int(g2[offs1[k] + start + 1])
    if to == 0 or to > offs2[-1]:
        return None
    k2 = int(np.searchsorted(offs2, to, side='left')) - 1
    start2 = to - int(offs2[k2]) - 1
    return (names2[k2], str(start2), str(start2 + 1), strand if not flip[offs1[k] + start + 1] else '+-'[strand == '+'])


def _contigs(fai):
    """read_fai's result, or a path -> ({name: index of the first contig of that name}, lens, offs, names)."""
    names, lens, offs = read_fai(fai) if isinstance(fai, (str, os.PathLike)) else fai
    index = {}
    for k, name in enumerate(names):
        index.setdefault(name, k)
    return index, lens, offs, list(names)


def _rows(bed1, bed2, xmfa_path=None, fai1=None, fai2=None, seqs=(1, 2), fisher=False, fdr=False):
    """-> the rows as bytes, their number, and (with an alignment) the keys of bed1 that have no image, else None."""
    sites1, sites2 = read_bed(bed1), read_bed(bed2)
    rows = []
    extra = _Extra(bed1, bed2, fisher, fdr) if fisher or fdr else None

    def add(pos, image, lifted):
        (frac1, depth1), x = sites1[pos]
        (frac2, depth2), y = sites2[image]
        head = list(pos) + (list(image) if lifted else []) + [frac1, depth1, frac2, depth2]
        if extra is None:
            rows.append('\t'.join(head + site_values(x, y)) + '\n')
            return
        logs = extra.site()
        fields = head + site_values(x, y, logs)
        if fisher:
            fields.append(extra.fisher_column(logs, pos, image, sites1[pos], sites2[image]))
        rows.append(fields)

    def done(n_unaligned):
        if extra is not None:
            extra.finish(rows)
            rows[:] = ['\t'.join(fields) + '\n' for fields in rows]
        return ''.join(rows).encode('utf-8', 'surrogateescape'), len(rows), n_unaligned

    if xmfa_path is None:
        for pos in sites1:
            if pos in sites2:
                add(pos, pos, False)
        return done(None)
    if fai1 is None or fai2 is None:
        raise ValueError('an alignment needs the .fai of both genomes')
    contigs1, contigs2 = _contigs(fai1), _contigs(fai2)
    g2, flip = xmfa_map(xmfa_path, int(contigs1[2][-1]), seqs, int(contigs2[2][-1]))
    n_unaligned = 0
    for pos in sites1:
        image = lift_key(pos, contigs1, contigs2, g2, flip)
        if image is None:
            n_unaligned += 1
        elif image in sites2:
            add(pos, image, True)
    return done(n_unaligned)


def compare_rows(bed1, bed2, xmfa_path=None, fai1=None, fai2=None, seqs=(1, 2), fisher=False, fdr=False):
    """The rows of the definition as bytes, and their number."""
    return _rows(bed1, bed2, xmfa_path, fai1, fai2, seqs, fisher, fdr)[:2]


def _done(by, reason, n_sites, n_unaligned, fisher=False, fdr=False):
    global last_compare
    last_compare = dict(by=by, reason=reason, n_sites=n_sites)
    if n_unaligned is not None:
        last_compare['n_unaligned'] = n_unaligned
    if fisher or fdr:                             # (a comparison without the flags says what it always said)
        last_compare.update(fisher=bool(fisher), fdr=bool(fdr))
    return n_sites


def _host(bed1, bed2, out, reason, lift=()):
    global last_compare
    last_compare = None
    data, n_sites, n_unaligned = _rows(bed1, bed2, *lift)
    _write(out, data)
    return _done('host', reason, n_sites, n_unaligned, *lift[4:6])


def compare_by_position(bed1, bed2, xmfa=None, out=None, xmfa_path=None, fai1=None, fai2=None, seqs=(1, 2), fisher=False, fdr=False):
    """The host statement: the definition above, one SciPy call after the other.  xmfa (-g) is accepted and unused; the
    alignment is xmfa_path."""
    return _host(bed1, bed2, out, 'the host statement was asked for', (xmfa_path, fai1, fai2, seqs, fisher, fdr))


def compare_by_position_device(bed1, bed2, xmfa=None, out=None, xmfa_path=None, fai1=None, fai2=None, seqs=(1, 2), fisher=False, fdr=False):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_compare
    from .device import get_device
    last_compare = None
    lift = (xmfa_path, fai1, fai2, seqs, fisher, fdr)
    flags = dict(fisher=True) if fisher else {}
    if fdr:
        flags['fdr'] = True
    if xmfa_path is None:
        blob, n_sites, reason = get_device().bed_compare(path1=bed1, path2=bed2, **flags)
        n_unaligned = None
    else:
        if fai1 is None or fai2 is None:
            raise ValueError('an alignment needs the .fai of both genomes')
        dev, contigs1, contigs2 = get_device(), read_fai(fai1), read_fai(fai2)
        if int(seqs[0]) == int(seqs[1]):
            raise ValueError('xmfa_map: two different sequence numbers')
        _, _, reason = dev.xmfa_map(path=xmfa_path, n1=int(contigs1[2][-1]), n2=int(contigs2[2][-1]), seqs=seqs, view=False)
        if reason is not None:
            return _host(bed1, bed2, out, reason, lift)
        try:
            blob, n_sites, reason = dev.bed_compare(path1=bed1, path2=bed2, contigs1=contigs1, contigs2=contigs2, **flags)
        finally:
            dev.xmfa_map_release()
        n_unaligned = dev.bed_compare_last_unaligned()
    if blob is None:
        return _host(bed1, bed2, out, reason, lift)
    _write(out, blob)
    return _done('device', None, n_sites, n_unaligned, fisher, fdr)


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Compare methylation between two genomes by probabilities of methylation for aligned positions')
    parser.add_argument('--bed1', type=str, required=False, help='bed file 1 with verbose output from make_bed.py')
    parser.add_argument('--bed2', type=str, required=False, help='bed file 2 with verbose output from make_bed.py')
    parser.add_argument('-g', '--genome_alignment', type=str, required=False,
                        help='an xmfa file from mauve (if absent, alignments assumed to be to the same reference genome)')
    parser.add_argument('--xmfa', type=str, required=False, help='compare through this Mauve alignment (needs --fai1 and --fai2)')
    parser.add_argument('--fai1', type=str, required=False, help="the .fai of bed1's genome")
    parser.add_argument('--fai2', type=str, required=False, help="the .fai of bed2's genome")
    parser.add_argument('--xmfa_seqs', type=str, default='1,2', help="the alignment's sequence numbers of bed1's and bed2's genome (default 1,2)")
    parser.add_argument('-o', '--output', type=str, required=False, help='write the rows to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', required=False, help='make the rows on the GPU (the host statement runs when it declines)')
    parser.add_argument('--fisher', action='store_true', required=False, help="append nlp_fisher: Fisher's exact test on the two lines' counts")
    parser.add_argument('--fdr', action='store_true', required=False, help='append the Benjamini-Hochberg q-value (-log10) of every p-value column')
    parser.add_argument('-v', '--version', action='store_true', required=False, help='print version')
    args = parser.parse_args(argv)

    if args.version:
        print('mCallerNP 0.3')
        sys.exit(0)
    if args.bed1 is None or args.bed2 is None:
        parser.error('the following arguments are required: --bed1, --bed2')

    assert os.path.isfile(args.bed1), 'file not found at ' + args.bed1
    assert os.path.isfile(args.bed2), 'file not found at ' + args.bed2

    run = compare_by_position_device if args.device else compare_by_position
    if args.fisher or args.fdr:
        run = functools.partial(run, fisher=args.fisher, fdr=args.fdr)
    if args.xmfa is None:
        run(args.bed1, args.bed2, args.genome_alignment, args.output)
        return
    if args.fai1 is None or args.fai2 is None:
        parser.error('--xmfa needs --fai1 and --fai2')
    seqs = args.xmfa_seqs.split(',')
    if len(seqs) != 2 or not all(plain_digits(s) for s in seqs) or seqs[0] == seqs[1]:
        parser.error('--xmfa_seqs: two different sequence numbers, as in 1,2')
    for path in (args.xmfa, args.fai1, args.fai2):
        assert os.path.isfile(path), 'file not found at ' + path
    run(args.bed1, args.bed2, args.genome_alignment, args.output, xmfa_path=args.xmfa, fai1=args.fai1, fai2=args.fai2,
        seqs=(int(seqs[0]), int(seqs[1])))


if __name__ == '__main__':
    main()
