"""Compare a native sample with an unmodified control site by site WITHOUT a trained model: do the two samples' current deviations
at a site come from the same distribution?

    python -m mcaller_amd.compare_currents --native A.diffs.6 --control B.diffs.6
        [-d 15] [--fdr] [--sig_bed OUT.bed --by {mwu,rs,t,ks} --threshold 2.0] [-o OUT] [--device]

The reference has no such program: everything it offers behind the scan starts from a classifier's probability.  The two inputs are
the rows `mCaller -m A` writes for the native DNA and for a whole-genome amplified control run through the same scan; the output
feeds `find_motifs --bed`, so "two eventalign files -> which motifs are modified" needs no model.

LINES.  A line of either file is split at tabs, as make_bed does (str.split('\\t') of the line with its newline).  Exactly 8 fields
are a predict row, exactly 7 a --train row: chrom, read, pos, context, values, strand, label[, probability]; anything else is
ValueError('<file> line <no>: ...').  The key is (chrom, pos as text, strand).  pos must be what int() takes (ValueError otherwise);
int(pos) + 1 is printed as the end.
VALUES.  [float(v) for v in values.split(',')][:-1]: the last number, the read quality, is parsed (float() is called on it) and not
tested.  The number of values nv of every row of both files is that of the native file's first row and at least 2, else ValueError
naming file and line; a number float() does not take is one too.  c = nv - 1 value columns are tested.  Every line of the native file
is checked in file order, then every line of the control file; on a line the field count comes first, then the numbers, their count, pos.
SITES are the keys of the native file in the order of their first row.  A site is kept when the control file has the key too and both
have at least -d rows (-d >= 2).  A site's rows stand in file order, per file; the printed context is that of its first native row.
PER SITE AND COLUMN j: compare_genomes.site_values(x_j, y_j, logs) gives t_j (ttest_ind's statistic, np.round(., 3)) and the four
unrounded log10 p: Mann-Whitney (two-sided, asymptotic), rank-sum, Student, Kolmogorov-Smirnov (Smirnov's limit).
COMBINING THE COLUMNS: per test by Bonferroni, which holds under any dependence between overlapping slots:
    L = min(0.0, min_j L_j + log10c), log10c = float(np.log10(c))            nlp = str(np.round(0.0 - L, 3))
(np.minimum and np.min: a NaN column makes the test's L NaN and prints nan).
ROW, tab-separated, one per kept site:

    chrom pos pos+1 context strand n_native n_control t_1 .. t_c nlp_mwu nlp_rs nlp_t nlp_ks [nlq_mwu nlq_rs nlq_t nlq_ks]

--fdr appends the nlq columns: compare_genomes.bh_log10 per test over the rows written, on the unrounded L, printed as
str(np.round(0.0 - Q, 3)).
--sig_bed OUT --by X --threshold T: every written row whose PRINTED nlp_X (with --fdr: nlq_X) is at least T also goes to OUT as

    chrom pos pos+1 context nlp strand n_native

which find_motifs --bed reads unchanged (fields 1, 2 and 6).  The decision is made on the printed value, so equal rows give equal
files; nan is not at least anything.
SciPy's nan sites (fewer than 3 pooled values, a zero pooled variance, a column whose pooled values are all equal) print as SciPy gives
them here; the device declines them, as it does for compare_genomes.

`compare_currents` is that definition written with the SciPy calls (the host statement).  `compare_currents_device` (--device) has
the GPU make the same bytes from the two texts (Device.currents_compare: csrc/compare/mc_sitegroup.inc, mc_curcompare.inc, csrc/mc_curcombine.h) and
runs the host statement whenever the device declines; `last_compare` says who made the output: dict(by='device' | 'host',
reason=None | str, n_sites=int, n_sig=int)."""
import os
import sys

import numpy as np

from .compare_genomes import _write, bh_log10, site_values

TESTS = ('mwu', 'rs', 't', 'ks')

last_compare = None


def read_rows(path, nv=None, min_values=2, labels=False):
    """{(chrom, pos, strand): [context of the first row, [values of a row, ...]]} of a .diffs file in the order of the keys' first rows,
    and the number of values of a row (nv: what it has to be, None: that of the first row).  labels (cluster_sites): a third list per
    site, True where the row's label starts with 'm', and a value that is not finite is a ValueError too."""
    sites = {}
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
            if len(values) != nv or nv < min_values:
                raise ValueError('%s line %d: %d values, %s' % (path, no, len(values), 'at least %d are needed' % min_values if nv < min_values
                                                                else '%d are expected' % nv))
            if labels and not all(v - v == 0.0 for v in values):
                raise ValueError('%s line %d: a value that is not finite' % (path, no))
            try:
                int(f[2])
            except ValueError:
                raise ValueError('%s line %d: a position that is no integer' % (path, no))
            site = sites.setdefault((f[0], f[2], f[5]), [f[3], [], []] if labels else [f[3], []])
            site[1].append(values[:-1])
            if labels:
                site[2].append(f[6][:1] == 'm')
    return sites, nv


def combine(logs, log10c):
    """L of the definition for one test: logs the c columns' unrounded log10 p."""
    with np.errstate(all='ignore'):
        return np.minimum(0.0, np.min(np.asarray(logs, dtype=np.float64)) + log10c)


def _rows(native, control, depth=15, fdr=False, by='mwu', threshold=2.0, want_bed=False):
    """-> (the rows as bytes, the bed's lines as bytes or None, rows written, rows in the bed)."""
    depth = int(depth)
    if depth < 2:
        raise ValueError('compare_currents: -d is at least 2')
    if by not in TESTS:
        raise ValueError('compare_currents: --by is one of mwu, rs, t, ks')
    nat, nv = read_rows(native)
    con, _ = read_rows(control, nv) if nv is not None else ({}, None)
    rows, L_all = [], []
    if nv is not None:
        c = nv - 1
        log10c = float(np.log10(c))
        for key, (context, x_rows) in nat.items():
            if key not in con or len(x_rows) < depth or len(con[key][1]) < depth:
                continue
            x = np.ascontiguousarray(np.asarray(x_rows, dtype=np.float64).T)   # [c, n]: a column is one contiguous run
            y = np.ascontiguousarray(np.asarray(con[key][1], dtype=np.float64).T)
            ts, logs = [], []
            for j in range(c):
                col = []
                ts.append(site_values(x[j], y[j], col)[3])
                logs.append(col)
            L = [combine([col[i] for col in logs], log10c) for i in range(4)]
            L_all.append(L)
            with np.errstate(all='ignore'):
                nlp = [str(np.round(0.0 - v, 3)) for v in L]
            chrom, pos, strand = key
            rows.append([chrom, pos, str(int(pos) + 1), context, strand, str(len(x_rows)), str(len(con[key][1]))] + ts + nlp)
    first = 7 + (nv - 1 if nv else 0)                                  # the column of nlp_mwu
    if fdr and rows:
        with np.errstate(all='ignore'):
            for L in np.asarray(L_all, dtype=np.float64).reshape(len(rows), 4).T:
                for fields, q in zip(rows, bh_log10(L)):
                    fields.append(str(np.round(0.0 - q, 3)))
        first += 4
    bed = None
    n_sig = 0
    if want_bed:
        col = first + TESTS.index(by)
        lines = ['\t'.join(f[:4] + [f[col], f[4], f[5]]) + '\n' for f in rows if float(f[col]) >= threshold]
        n_sig = len(lines)
        bed = ''.join(lines).encode('utf-8', 'surrogateescape')
    data = ''.join('\t'.join(f) + '\n' for f in rows).encode('utf-8', 'surrogateescape')
    return data, bed, len(rows), n_sig


def compare_rows(native, control, depth=15, fdr=False):
    """The rows of the definition as bytes, and their number."""
    data, _, n, _ = _rows(native, control, depth, fdr)
    return data, n


def _done(by, reason, n_sites, n_sig):
    global last_compare
    last_compare = dict(by=by, reason=reason, n_sites=n_sites, n_sig=n_sig)
    return n_sites


def _host(native, control, out, reason, depth, fdr, sig_bed, by, threshold):
    global last_compare
    last_compare = None
    data, bed, n_sites, n_sig = _rows(native, control, depth, fdr, by, threshold, sig_bed is not None)
    _write(out, data)
    if sig_bed is not None:
        _write(sig_bed, bed)
    return _done('host', reason, n_sites, n_sig)


def compare_currents(native, control, out=None, depth=15, fdr=False, sig_bed=None, by='mwu', threshold=2.0):
    """The host statement: the definition above, one SciPy call after the other."""
    return _host(native, control, out, 'the host statement was asked for', depth, fdr, sig_bed, by, threshold)


def compare_currents_device(native, control, out=None, depth=15, fdr=False, sig_bed=None, by='mwu', threshold=2.0):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_compare
    from .device import get_device
    last_compare = None
    if int(depth) < 2:
        raise ValueError('compare_currents: -d is at least 2')
    if by not in TESTS:
        raise ValueError('compare_currents: --by is one of mwu, rs, t, ks')
    blob, bed, n_sites, n_sig, reason = get_device().currents_compare(path1=native, path2=control, depth=int(depth), fdr=fdr,
                                                                      by=by if sig_bed is not None else None, threshold=threshold)
    if blob is None:
        return _host(native, control, out, reason, depth, fdr, sig_bed, by, threshold)
    _write(out, blob)
    if sig_bed is not None:
        _write(sig_bed, bed)
    return _done('device', None, n_sites, n_sig)


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Compare the current deviations of a native sample and an unmodified control site by site, without a model')
    parser.add_argument('--native', type=str, required=True, help='mCaller rows (.diffs) of the native sample')
    parser.add_argument('--control', type=str, required=True, help='mCaller rows (.diffs) of the unmodified control')
    parser.add_argument('-d', '--min_depth', type=int, default=15, help='rows a site needs in each file (default 15, at least 2)')
    parser.add_argument('--fdr', action='store_true', help='append the Benjamini-Hochberg q-value (-log10) of every p-value column')
    parser.add_argument('--sig_bed', type=str, required=False, help='write the significant sites to this BED file (for find_motifs --bed)')
    parser.add_argument('--by', type=str, default='mwu', choices=TESTS, help='the test --sig_bed goes by (default mwu)')
    parser.add_argument('--threshold', type=float, default=2.0, help='--sig_bed takes a printed -log10 p (with --fdr: q) of at least this (default 2.0)')
    parser.add_argument('-o', '--output', type=str, required=False, help='write the rows to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', help='make the rows on the GPU (the host statement runs when it declines)')
    args = parser.parse_args(argv)
    if args.min_depth < 2:
        parser.error('-d: at least 2 rows a site and file')
    assert os.path.isfile(args.native), 'file not found at ' + args.native
    assert os.path.isfile(args.control), 'file not found at ' + args.control
    run = compare_currents_device if args.device else compare_currents
    run(args.native, args.control, args.output, depth=args.min_depth, fdr=args.fdr, sig_bed=args.sig_bed, by=args.by, threshold=args.threshold)
    if args.device and last_compare['by'] == 'host':
        print('compare_currents: %s; the host statement made the output' % last_compare['reason'], file=sys.stderr)


if __name__ == '__main__':
    main()
