"""Split the reads of every site in two by their currents alone and set the split beside the classifier's labels: is the site a
mixture (phase-variable methyltransferases, hemimethylation, partial modification), and does the classifier part the reads where
the currents part them?

    python -m mcaller_amd.cluster_sites -f reads.eventalign.diffs.6 [-d 15] [--max_depth 256]
        [--metric {correlation,euclidean}] [--mixed_bed OUT.bed --min_minor 0.2 --min_gap 2.0] [-o OUT] [--device]

The reference's make_bed.py:50-64, cluster(), links a site's reads by the correlation distance of their current vectors (complete
linkage), cuts the tree in two and plots the clusters beside the labels; plotlib.plot_w_labels prints their adjusted Rand index.
Where this leaves the reference: the condensed distances go to the linkage here, not the square distance matrix as if its rows were
observations, and nothing is plotted -- the numbers are the output, one row per site.

LINES are compare_currents' (read_rows): split at tabs, exactly 7 or 8 fields (chrom, read, pos, context, values, strand,
label[, probability]), anything else is ValueError('<file> line <no>: ...').  The key is (chrom, pos as text, strand); pos must be
what int() takes.  VALUES.  [float(v) for v in values.split(',')][:-1]; every line has the value count of the first row and at least
3 values (c >= 2 columns), else ValueError; a value that is not finite is a ValueError naming file and line.  A row is methylated
when its label starts with 'm'.
SITES are the keys in the order of their first rows.  A site's rows are its first --max_depth rows in file order (2 <= max_depth <=
1024); later rows are counted in n and otherwise ignored.  Under `correlation` a row is FLAT, and left out, when its centred sum of
squares q is 0 or not finite; under `euclidean` no row is flat.  A site is kept when its usable rows number at least -d (d >= 2).
DISTANCE, in fp64, every operation in the stated order, none contracted (v the c values of a row):
    correlation   m = (((v0 + v1) + v2) + ...) / c      w_k = v_k - m      q = ((w0 w0 + w1 w1) + ...)      u_k = w_k / sqrt(q)
                  d(a, b) = max(0.0, 1.0 - (((u_a0 u_b0) + u_a1 u_b1) + ...))
    euclidean     d(a, b) = sqrt(((e0 e0 + e1 e1) + ...)),  e_k = a_k - b_k
LINKAGE.  From singletons, until two clusters are left, merge the pair (A, B) with the smallest D(A, B) = max d(a, b) over a in A, b
in B; among equal distances the pair whose (smallest row index in A, smallest row index in B) is lexicographically smallest, A the
cluster with the smaller index.  The rule is total: ties never decline.  Cluster 1 holds the site's first usable row, cluster 2 is
the other.  h_top is the distance at which the last two would merge, h_sub the larger of the two clusters' own last merge distances
(a singleton: 0.0).
AGREEMENT.  From the 2 x 2 counts of (cluster, methylated) the pair counts tn, fp, fn, tp, Python integers: ari = 1.0 when fn == 0
and fp == 0, else float(2 (tp tn - fn fp)) / float((tp + fn) (fn + tn) + (tp + fp) (fp + tn)); printed as str(np.round(ari, 3)).
ROW, tab-separated, one per kept site (n_i the rows of cluster i, m_i the methylated among them; h_* as repr()):

    chrom pos pos+1 context strand n n_flat n_1 n_2 m_1 m_2 h_top h_sub ari

--mixed_bed OUT --min_minor F --min_gap G: a written row also goes to OUT when min(n_1, n_2) / (n_1 + n_2) >= F (one division) and
h_top >= G * h_sub (one multiplication), as

    chrom pos pos+1 context h_top strand n

which find_motifs --bed reads unchanged.

`cluster_sites` is that definition in NumPy, column by column (the host statement).  `cluster_sites_device` (--device) has the GPU
make the same bytes from the text (Device.sites_cluster: csrc/compare/mc_sitegroup.inc, mc_sitecluster.inc, csrc/mc_linkage.h) and runs the host
statement whenever the device declines; `last_cluster` says who made the output: dict(by='device' | 'host', reason=None | str,
n_sites=int, n_mixed=int)."""
import os
import sys

import numpy as np

from .compare_currents import read_rows
from .compare_genomes import _write

METRICS = ('correlation', 'euclidean')
MAX_DEPTH = 1024

last_cluster = None


def usable_rows(X, metric):
    """X [n, c] -> (the vectors the distance is taken between -- u under correlation, the rows themselves under euclidean --, the
    indices of the usable rows)."""
    X = np.asarray(X, dtype=np.float64)
    n, c = X.shape
    if metric == 'euclidean':
        return X, np.arange(n)
    with np.errstate(all='ignore'):
        m = X[:, 0]
        for k in range(1, c):
            m = m + X[:, k]
        m = m / float(c)
        w = [X[:, k] - m for k in range(c)]
        q = w[0] * w[0]
        for k in range(1, c):
            q = q + w[k] * w[k]
        keep = np.flatnonzero(np.isfinite(q) & (q != 0.0))
        s = np.sqrt(q[keep])
        U = np.empty((len(keep), c), dtype=np.float64)
        for k in range(c):
            U[:, k] = w[k][keep] / s
    return U, keep


def distances(U, metric):
    """The square matrix of d(a, b) over the rows of U (the diagonal is not used)."""
    n, c = U.shape
    with np.errstate(all='ignore'):
        if metric == 'euclidean':
            e = U[:, None, 0] - U[None, :, 0]
            acc = e * e
            for k in range(1, c):
                e = U[:, None, k] - U[None, :, k]
                acc = acc + e * e
            return np.sqrt(acc)
        acc = U[:, None, 0] * U[None, :, 0]
        for k in range(1, c):
            acc = acc + U[:, None, k] * U[None, :, k]
        return np.maximum(0.0, 1.0 - acc)


def link_two(D):
    """Complete linkage of the definition on the square matrix D (n >= 2) down to two clusters -> (labels: 1 where a row is in the
    cluster of row 0, else 2; h_top; h_sub)."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    alive = np.ones(n, dtype=bool)
    member = np.arange(n)
    height = np.zeros(n, dtype=np.float64)
    nn_d = np.zeros(n, dtype=np.float64)
    nn_j = np.full(n, -1)

    def nearest(i):                                   # the smallest D[i, j] over the living j > i, the smallest such j
        js = i + 1 + np.flatnonzero(alive[i + 1:])
        if len(js) == 0:
            nn_j[i] = -1
            return
        k = int(np.argmin(D[i, js]))
        nn_j[i] = js[k]
        nn_d[i] = D[i, js[k]]

    for i in range(n):
        nearest(i)
    for _ in range(n - 2):
        rows = np.flatnonzero(alive & (nn_j >= 0))
        a = int(rows[np.argmin(nn_d[rows])])          # the first of equal minima: the smallest index in A, then nn_j: in B
        b = int(nn_j[a])
        height[a] = nn_d[a]
        merged = np.maximum(D[a], D[b])
        D[a, :] = merged
        D[:, a] = merged
        alive[b] = False
        member[member == b] = a
        for i in np.flatnonzero(alive & ((nn_j == a) | (nn_j == b))):
            nearest(int(i))
        nearest(a)
    other = int(np.flatnonzero(alive)[1])
    labels = np.where(member == 0, 1, 2)
    return labels, float(D[0, other]), float(max(height[0], height[other]))


def ari_of(n1, n2, m1, m2):
    """The adjusted Rand index of (cluster, methylated) from the sizes of the two clusters and the methylated rows in each."""
    n = n1 + n2
    cells = (m1, n1 - m1, m2, n2 - m2)
    ss = sum(v * v for v in cells)
    tp = ss - n
    fp = n1 * n1 + n2 * n2 - ss
    fn = (m1 + m2) ** 2 + (n - m1 - m2) ** 2 - ss
    tn = n * n - fp - fn - ss
    if fn == 0 and fp == 0:
        return 1.0
    num, den = 2 * (tp * tn - fn * fp), (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)
    assert abs(num) < 2 ** 53 and 0 < den < 2 ** 53
    return float(num) / float(den)


def site_split(X, meth, metric='correlation'):
    """One site: X [rows, c] (the first max_depth rows), meth their labels -> None when fewer than 2 rows are usable, else
    (n_flat, n_1, n_2, m_1, m_2, h_top, h_sub, ari, labels of the usable rows)."""
    U, keep = usable_rows(X, metric)
    if len(keep) < 2:
        return None
    labels, h_top, h_sub = link_two(distances(U, metric))
    meth = np.asarray(meth, dtype=bool)[keep]
    n1, n2 = int(np.sum(labels == 1)), int(np.sum(labels == 2))
    m1, m2 = int(np.sum(meth & (labels == 1))), int(np.sum(meth & (labels == 2)))
    return len(X) - len(keep), n1, n2, m1, m2, h_top, h_sub, ari_of(n1, n2, m1, m2), labels


def _check(depth, max_depth, metric):
    if int(depth) < 2:
        raise ValueError('cluster_sites: -d is at least 2')
    if not 2 <= int(max_depth) <= MAX_DEPTH:
        raise ValueError('cluster_sites: --max_depth is 2 to %d' % MAX_DEPTH)
    if metric not in METRICS:
        raise ValueError('cluster_sites: --metric is correlation or euclidean')


def _rows(path, depth=15, max_depth=256, metric='correlation', want_bed=False, min_minor=0.2, min_gap=2.0):
    """-> (the rows as bytes, the bed's lines as bytes or None, rows written, rows in the bed)."""
    _check(depth, max_depth, metric)
    depth, max_depth = int(depth), int(max_depth)
    sites, _ = read_rows(path, min_values=3, labels=True)
    rows, bed = [], []
    for (chrom, pos, strand), (context, values, meth) in sites.items():
        if len(values) < depth:
            continue
        got = site_split(values[:max_depth], meth[:max_depth], metric)
        if got is None or got[1] + got[2] < depth:
            continue
        n_flat, n1, n2, m1, m2, h_top, h_sub, ari = got[:8]
        head = [chrom, pos, str(int(pos) + 1), context]
        rows.append('\t'.join(head + [strand] + [str(v) for v in (len(values), n_flat, n1, n2, m1, m2)] +
                              [repr(h_top), repr(h_sub), str(np.round(ari, 3))]) + '\n')
        if want_bed and float(min(n1, n2)) / float(n1 + n2) >= min_minor and h_top >= min_gap * h_sub:
            bed.append('\t'.join(head + [repr(h_top), strand, str(len(values))]) + '\n')
    data = ''.join(rows).encode('utf-8', 'surrogateescape')
    return data, (''.join(bed).encode('utf-8', 'surrogateescape') if want_bed else None), len(rows), len(bed)


def _done(by, reason, n_sites, n_mixed):
    global last_cluster
    last_cluster = dict(by=by, reason=reason, n_sites=n_sites, n_mixed=n_mixed)
    return n_sites


def _host(path, out, reason, depth, max_depth, metric, mixed_bed, min_minor, min_gap):
    global last_cluster
    last_cluster = None
    data, bed, n_sites, n_mixed = _rows(path, depth, max_depth, metric, mixed_bed is not None, float(min_minor), float(min_gap))
    _write(out, data)
    if mixed_bed is not None:
        _write(mixed_bed, bed)
    return _done('host', reason, n_sites, n_mixed)


def cluster_sites(path, out=None, depth=15, max_depth=256, metric='correlation', mixed_bed=None, min_minor=0.2, min_gap=2.0):
    """The host statement: the definition above in NumPy."""
    return _host(path, out, 'the host statement was asked for', depth, max_depth, metric, mixed_bed, min_minor, min_gap)


def cluster_sites_device(path, out=None, depth=15, max_depth=256, metric='correlation', mixed_bed=None, min_minor=0.2, min_gap=2.0):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_cluster
    from .device import get_device
    last_cluster = None
    _check(depth, max_depth, metric)
    blob, bed, n_sites, n_mixed, reason = get_device().sites_cluster(path=path, depth=int(depth), max_depth=int(max_depth), metric=metric,
                                                                     mixed=mixed_bed is not None, min_minor=float(min_minor),
                                                                     min_gap=float(min_gap))
    if blob is None:
        return _host(path, out, reason, depth, max_depth, metric, mixed_bed, min_minor, min_gap)
    _write(out, blob)
    if mixed_bed is not None:
        _write(mixed_bed, bed)
    return _done('device', None, n_sites, n_mixed)


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Split the reads of every site in two by their currents and set the split beside the labels')
    parser.add_argument('-f', '--file', type=str, required=True, help='mCaller rows (.diffs)')
    parser.add_argument('-d', '--min_depth', type=int, default=15, help='usable rows a site needs (default 15, at least 2)')
    parser.add_argument('--max_depth', type=int, default=256, help='rows of a site that are clustered, the first in the file (default 256, 2 to 1024)')
    parser.add_argument('--metric', type=str, default='correlation', choices=METRICS, help='the distance between two rows (default correlation)')
    parser.add_argument('--mixed_bed', type=str, required=False, help='write the sites that look like mixtures to this BED file (for find_motifs --bed)')
    parser.add_argument('--min_minor', type=float, default=0.2, help='--mixed_bed: the smaller cluster holds at least this share of the rows (default 0.2)')
    parser.add_argument('--min_gap', type=float, default=2.0, help='--mixed_bed: h_top is at least this many times h_sub (default 2.0)')
    parser.add_argument('-o', '--output', type=str, required=False, help='write the rows to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', help='make the rows on the GPU (the host statement runs when it declines)')
    args = parser.parse_args(argv)
    if args.min_depth < 2:
        parser.error('-d: at least 2 usable rows a site')
    if not 2 <= args.max_depth <= MAX_DEPTH:
        parser.error('--max_depth: 2 to %d' % MAX_DEPTH)
    assert os.path.isfile(args.file), 'file not found at ' + args.file
    run = cluster_sites_device if args.device else cluster_sites
    run(args.file, args.output, depth=args.min_depth, max_depth=args.max_depth, metric=args.metric, mixed_bed=args.mixed_bed,
        min_minor=args.min_minor, min_gap=args.min_gap)
    if args.device and last_cluster['by'] == 'host':
        print('cluster_sites: %s; the host statement made the output' % last_cluster['reason'], file=sys.stderr)


if __name__ == '__main__':
    main()
