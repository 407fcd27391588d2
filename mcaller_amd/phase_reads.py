"""Methylation linkage between sites along reads: do two sites change state together on the same molecule?

    python -m mcaller_amd.phase_reads -f reads.diffs.6 [-d 15] [--max_dist 1000] [--min_reads 10] [--min_margin 2]
        [--fdr] [--reads OUT.reads] [--linked_bed OUT.bed --threshold 2.0] [-o OUT] [--device]

The reference has no such program: everything it offers behind the scan answers a question about a single site.  cluster_sites can
say that a site is a mixture; this says whether two mixed sites are the SAME mixture (a phase-variable methyltransferase, a mixed
population).  The input is the rows `mCaller -m A` writes; --linked_bed feeds `find_motifs --bed`, as --sig_bed and --mixed_bed do.

LINES.  compare_currents.read_rows' rules, unchanged, with min_values=2: a line is split at tabs (str.split('\\t') of the line with
its newline); exactly 8 fields are a predict row, exactly 7 a --train row: chrom, read, pos, context, values, strand, label[,
probability]; anything else is ValueError('<file> line <no>: ...').  float() is called on every value (ValueError: a value that is
no number); the number of values of every row is that of the first row and at least 2 (ValueError naming the count); pos must be
what int() takes (ValueError).  On a line the field count comes first, then the numbers, their count, pos.  A row is METHYLATED when
label[:1] == 'm'.
KEYS.  A site is (chrom, pos as text, strand); a read is (chrom, read, strand).
CALLS.  A call is the first row in file order of a (read key, pos as text) combination.  Later rows of the combination are
duplicates: they are counted in last_phase['n_duplicates'] and otherwise ignored.
SITES.  N of a site is the number of its calls; a site is KEPT when N >= -d.  Sites are numbered in the order of their first rows.
PAIRS.  A pair (A, B) is two kept sites of one chrom and strand with 0 < int(posB) - int(posA) <= --max_dist.  Its shared reads are
the read keys with a call at both; n is their number, and n11, n10, n01, n00 count them by (A methylated, B methylated).
ROWS.  A pair is written iff n >= --min_reads and each of the four margins n11 + n10, n01 + n00, n11 + n01, n10 + n00 is at least
--min_margin: no written table is degenerate.
VALUES, in these fp64 operations (the integer products are exact below 2^53):

    phi = float(n11 * n00 - n10 * n01) / (sqrt(float((n11 + n10) * (n01 + n00))) * sqrt(float((n11 + n01) * (n10 + n00))))
    L = compare_genomes.fisher_log10p(n11, n11 + n10, n01, n01 + n00)

printed as str(np.round(phi, 3)) and str(np.round(0.0 - L, 3)).  --fdr appends compare_genomes.bh_log10 of L over the rows written,
printed as str(np.round(0.0 - Q, 3)).
ROW, tab-separated:

    chrom strand posA posB n n11 n10 n01 n00 phi nlp_fisher [nlq_fisher]

ORDER.  By A in the sites' first-row order; within A by int(posB) ascending; equal ints under different texts go by B's first row.
--reads OUT: one row per read key with at least one call at a kept site, in the order of the reads' first rows:

    chrom read strand first_pos last_pos n_sites n_meth

over the read's calls at kept sites: the smallest and the largest int(pos), printed as str() of the int, the calls, the methylated.
--linked_bed OUT --threshold T: a kept site qualifies when it is A or B of at least one written pair whose PRINTED nlp_fisher (with
--fdr: nlq_fisher) is at least T; n_links is the number of such pairs.  The decision is made on the printed value.  The sites stand
in first-row order:

    chrom pos pos+1 context n_links strand N

(context: that of the site's first row), which find_motifs --bed reads unchanged (fields 1, 2 and 6).

ValueError, beside the lines': -d below 1, --max_dist below 1, --min_reads below 1, --min_margin below 1, a --threshold that is nan.

`phase_reads` is that definition in plain Python and NumPy (the host statement).  `phase_reads_device` (--device) has the GPU make
the same bytes from the text (Device.reads_phase: csrc/compare/mc_sitegroup.inc, mc_readphase.inc, csrc/mc_pairphase.h) and runs the
host statement whenever the device declines; `last_phase` says who made the output: dict(by='device' | 'host', reason=None | str,
n_sites=kept sites, n_pairs=rows written, n_reads=rows of --reads, n_linked=lines of the bed, n_duplicates=int; the device declines a
file with a duplicate wherever a site is kept, so its own figure is 0 -- a file without a kept site writes nothing and is not looked
through for duplicates)."""
import os
import sys
from math import sqrt

import numpy as np

from .compare_genomes import _write, bh_log10, fisher_log10p

last_phase = None


def check_options(depth, max_dist, min_reads, min_margin, threshold):
    if int(depth) < 1:
        raise ValueError('phase_reads: -d is at least 1')
    if int(max_dist) < 1:
        raise ValueError('phase_reads: --max_dist is at least 1')
    if int(min_reads) < 1:
        raise ValueError('phase_reads: --min_reads is at least 1')
    if int(min_margin) < 1:
        raise ValueError('phase_reads: --min_margin is at least 1')
    if float(threshold) != float(threshold):
        raise ValueError('phase_reads: --threshold is a number')


def read_calls(path):
    """-> (sites: {(chrom, pos, strand): [context of the first row, N]} in the order of the sites' first rows,
    reads: {(chrom, read, strand): {pos: methylated}} in the order of the reads' first rows, a read's calls in file order,
    duplicates).  The checks and their order are compare_currents.read_rows'."""
    sites, reads, duplicates, nv = {}, {}, 0, None
    with open(path, 'r') as fh:
        for no, line in enumerate(fh, 1):
            f = line.split('\t')
            if len(f) not in (7, 8):
                raise ValueError('%s line %d: %d tab-separated fields, an mCaller row has 7 or 8' % (path, no, len(f)))
            try:
                values = [float(v) for v in f[4].split(',')]
            except ValueError:
                raise ValueError('%s line %d: a value that is no number' % (path, no))
            if nv is None:
                nv = len(values)
            if len(values) != nv or nv < 2:
                raise ValueError('%s line %d: %d values, %s' % (path, no, len(values), 'at least 2 are needed' if nv < 2 else '%d are expected' % nv))
            try:
                int(f[2])
            except ValueError:
                raise ValueError('%s line %d: a position that is no integer' % (path, no))
            calls = reads.setdefault((f[0], f[1], f[5]), {})
            if f[2] in calls:
                duplicates += 1
                continue
            calls[f[2]] = f[6][:1] == 'm'
            sites.setdefault((f[0], f[2], f[5]), [f[3], 0])[1] += 1
    return sites, reads, duplicates


def phi_of(n11, n10, n01, n00):
    """phi of the definition: Python ints, math.sqrt and the fp64 division."""
    return float(n11 * n00 - n10 * n01) / (sqrt(float((n11 + n10) * (n01 + n00))) * sqrt(float((n11 + n01) * (n10 + n00))))


def _rows(path, depth=15, max_dist=1000, min_reads=10, min_margin=2, fdr=False, threshold=2.0, want_reads=False, want_bed=False):
    """-> (the rows, the --reads rows or None, the bed's lines or None -- bytes --, dict(n_sites, n_pairs, n_reads, n_linked, n_duplicates))."""
    check_options(depth, max_dist, min_reads, min_margin, threshold)
    depth, max_dist, min_reads, min_margin = int(depth), int(max_dist), int(min_reads), int(min_margin)
    sites, reads, duplicates = read_calls(path)
    kept = [key for key, (_, n) in sites.items() if n >= depth]
    number = {key: i for i, key in enumerate(kept)}
    S = len(kept)
    positions = [int(key[1]) for key in kept]
    site_pos = np.asarray(positions, dtype=np.int64)
    # every read's calls at kept sites, ordered by int(pos): the pair instances as (A S + B) 4 + class, class = 2 (A unmethylated) + (B unmethylated)
    codes, read_rows = [], []
    for (chrom, read, strand), calls in reads.items():
        mine = [(number[(chrom, pos, strand)], meth) for pos, meth in calls.items() if (chrom, pos, strand) in number]
        if not mine:
            continue
        at = [positions[s] for s, _ in mine]
        read_rows.append('\t'.join((chrom, read, strand, str(min(at)), str(max(at)), str(len(mine)), str(sum(1 for _, m in mine if m)))) + '\n')
        if len(mine) < 2:
            continue
        idx = np.asarray([s for s, _ in mine], dtype=np.int64)
        meth = np.asarray([m for _, m in mine], dtype=np.int64)
        pos = site_pos[idx]
        order = np.argsort(pos, kind='stable')
        idx, meth, pos = idx[order], meth[order], pos[order]
        last = np.searchsorted(pos, pos + max_dist, side='right')       # the calls [first, last) behind call i lie within max_dist ...
        first = np.searchsorted(pos, pos, side='right')                 # ... and beyond its own position
        for i in np.flatnonzero(last > first):
            j = np.arange(first[i], last[i])
            codes.append(((idx[i] * S + idx[j]) << 2) | ((1 - meth[i]) << 1) | (1 - meth[j]))
    tables = {}
    if codes:
        code, count = np.unique(np.concatenate(codes), return_counts=True)
        for c, k in zip(code.tolist(), count.tolist()):
            tables.setdefault(c >> 2, [0, 0, 0, 0])[c & 3] = k
    written = []
    for ab, (n11, n10, n01, n00) in tables.items():
        if n11 + n10 + n01 + n00 >= min_reads and min(n11 + n10, n01 + n00, n11 + n01, n10 + n00) >= min_margin:
            a, b = divmod(ab, S)
            written.append((a, int(site_pos[b]), b, n11, n10, n01, n00))
    written.sort()
    rows, logs = [], []
    for a, _, b, n11, n10, n01, n00 in written:
        L = fisher_log10p(n11, n11 + n10, n01, n01 + n00)
        logs.append(L)
        chrom, pos_a, strand = kept[a]
        rows.append([chrom, strand, pos_a, kept[b][1]] + [str(v) for v in (n11 + n10 + n01 + n00, n11, n10, n01, n00)] +
                    [str(np.round(phi_of(n11, n10, n01, n00), 3)), str(np.round(0.0 - L, 3))])
    if fdr and rows:
        for fields, q in zip(rows, bh_log10(np.asarray(logs, dtype=np.float64))):
            fields.append(str(np.round(0.0 - q, 3)))
    bed, n_linked = None, 0
    if want_bed:
        links = [0] * S
        for (a, _, b, _, _, _, _), fields in zip(written, rows):
            if float(fields[-1]) >= threshold:
                links[a] += 1
                links[b] += 1
        lines = ['\t'.join((key[0], key[1], str(int(key[1]) + 1), sites[key][0], str(links[i]), key[2], str(sites[key][1]))) + '\n'
                 for i, key in enumerate(kept) if links[i] > 0]
        n_linked = len(lines)
        bed = ''.join(lines).encode('utf-8', 'surrogateescape')
    data = ''.join('\t'.join(f) + '\n' for f in rows).encode('utf-8', 'surrogateescape')
    reads_out = ''.join(read_rows).encode('utf-8', 'surrogateescape') if want_reads else None
    return data, reads_out, bed, dict(n_sites=S, n_pairs=len(rows), n_reads=len(read_rows), n_linked=n_linked, n_duplicates=duplicates)


def _done(by, reason, figures):
    global last_phase
    last_phase = dict(by=by, reason=reason, **figures)
    return figures['n_pairs']


def _host(path, out, reason, depth, max_dist, min_reads, min_margin, fdr, reads, linked_bed, threshold):
    global last_phase
    last_phase = None
    data, reads_out, bed, figures = _rows(path, depth, max_dist, min_reads, min_margin, fdr, threshold, reads is not None, linked_bed is not None)
    _write(out, data)
    if reads is not None:
        _write(reads, reads_out)
    if linked_bed is not None:
        _write(linked_bed, bed)
    return _done('host', reason, figures)


def phase_reads(path, out=None, depth=15, max_dist=1000, min_reads=10, min_margin=2, fdr=False, reads=None, linked_bed=None, threshold=2.0):
    """The host statement: the definition above in plain Python and NumPy -> the rows written."""
    return _host(path, out, 'the host statement was asked for', depth, max_dist, min_reads, min_margin, fdr, reads, linked_bed, threshold)


def phase_reads_device(path, out=None, depth=15, max_dist=1000, min_reads=10, min_margin=2, fdr=False, reads=None, linked_bed=None, threshold=2.0):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_phase
    from .device import get_device
    last_phase = None
    check_options(depth, max_dist, min_reads, min_margin, threshold)
    blob, reads_out, bed, n_pairs, n_reads, n_linked, reason = get_device().reads_phase(
        path=path, depth=int(depth), max_dist=int(max_dist), min_reads=int(min_reads), min_margin=int(min_margin), fdr=fdr,
        threshold=threshold if linked_bed is not None else None)
    if blob is None:
        return _host(path, out, reason, depth, max_dist, min_reads, min_margin, fdr, reads, linked_bed, threshold)
    n_sites = int(get_device().reads_phase_last_stats()['n_sites'])
    _write(out, blob)
    if reads is not None:
        _write(reads, reads_out)
    if linked_bed is not None:
        _write(linked_bed, bed)
    return _done('device', None, dict(n_sites=n_sites, n_pairs=n_pairs, n_reads=n_reads, n_linked=n_linked, n_duplicates=0))


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Test pairs of nearby sites for linked methylation over the reads that cover both')
    parser.add_argument('-f', '--file', type=str, required=True, help='mCaller rows (.diffs) of the sample')
    parser.add_argument('-d', '--min_depth', type=int, default=15, help='calls a site needs (default 15, at least 1)')
    parser.add_argument('--max_dist', type=int, default=1000, help='the largest distance between the two sites of a pair (default 1000)')
    parser.add_argument('--min_reads', type=int, default=10, help='shared reads a written pair needs (default 10)')
    parser.add_argument('--min_margin', type=int, default=2, help='the least each margin of a written table holds (default 2, at least 1)')
    parser.add_argument('--fdr', action='store_true', help='append the Benjamini-Hochberg q-value (-log10) of the p-value column')
    parser.add_argument('--reads', type=str, required=False, help='write one row per read with a call at a kept site to this file')
    parser.add_argument('--linked_bed', type=str, required=False, help='write the sites of significant pairs to this BED file (for find_motifs --bed)')
    parser.add_argument('--threshold', type=float, default=2.0, help='--linked_bed takes a printed -log10 p (with --fdr: q) of at least this (default 2.0)')
    parser.add_argument('-o', '--output', type=str, required=False, help='write the rows to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', help='make the rows on the GPU (the host statement runs when it declines)')
    args = parser.parse_args(argv)
    for name in ('min_depth', 'max_dist', 'min_reads', 'min_margin'):
        if getattr(args, name) < 1:
            parser.error('--%s: at least 1' % name)
    assert os.path.isfile(args.file), 'file not found at ' + args.file
    run = phase_reads_device if args.device else phase_reads
    run(args.file, args.output, depth=args.min_depth, max_dist=args.max_dist, min_reads=args.min_reads, min_margin=args.min_margin, fdr=args.fdr,
        reads=args.reads, linked_bed=args.linked_bed, threshold=args.threshold)
    if args.device and last_phase['by'] == 'host':
        print('phase_reads: %s; the host statement made the output' % last_phase['reason'], file=sys.stderr)


if __name__ == '__main__':
    main()
