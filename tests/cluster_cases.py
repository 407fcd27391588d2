"""The inputs of tests/test_cluster_sites.py and tests/test_gpu_cluster_sites.py, and the brute force both hold the host statement
against: .diffs rows of one sample, written out and seeded; the definition of cluster_sites as plain Python loops over clusters and
pairs, the tie rule letter by letter.  Nothing of mcaller_amd.cluster_sites is used here."""
import math

import numpy as np

from tests.currents_cases import interleave, row

C6 = 6


def gaussian(rng, n, c=C6, split=0.0, decimals=2):
    """n rows of c deviations; the second half of the rows shifted by `split` in the even columns (a planted second population)."""
    X = rng.normal(0.0, 1.0, size=(n, c))
    X[n // 2:, ::2] += split
    return np.round(X, decimals)


def integers(rng, n, c=C6, span=2):
    """small integers: equal distances are common, the index rule decides"""
    return rng.integers(-span, span + 1, size=(n, c)).astype(np.float64)


def site_lines(chrom, pos, strand, X, tag='r', labels=None, fields='mixed', context='GATCMGATCGA'):
    """The rows of one site in order; labels: 'm6A' / 'A' per row (default: the first third methylated); every other row has 7 fields
    under 'mixed', all under 7, none under 8."""
    out = []
    for i, v in enumerate(X):
        meth = labels[i] if labels is not None else i % 3 == 0
        prob = None if fields == 7 or (fields == 'mixed' and i % 2) else 0.75
        out.append(row(chrom, pos, strand, v, quality=8.0 + (i % 7) / 4, context=context, read='%s_%d' % (tag, i), label='m6A' if meth else 'A',
                       prob=prob))
    return out


def text_of(groups, rng=None):
    """The lines of the sites one after the other, or (rng) shuffled together with each site's own lines in their order."""
    return ''.join(interleave(groups, rng) if rng is not None else [l for g in groups for l in g]).encode()


def seeded_text(n_sites, lo, hi, seed, c=C6, shuffle=True, planted=4, maker=gaussian):
    """n_sites sites of lo .. hi rows (every `planted`-th with a second population), plus a site below any depth."""
    rng = np.random.default_rng([seed, n_sites])
    groups = []
    for s in range(n_sites):
        n = int(rng.integers(lo, hi + 1))
        X = maker(rng, n, c, 2.5 if planted and s % planted == 0 else 0.0) if maker is gaussian else maker(rng, n, c)
        labels = [bool(v) for v in (np.arange(n) >= n // 2 if planted and s % planted == 0 else rng.random(n) < 0.3)]
        groups.append(site_lines('chr1', 100 + 5 * s, '+-'[s & 1], X, 's%d' % s, labels))
    groups.append(site_lines('chr2', 7, '+', gaussian(rng, 1, c), 'x'))
    return text_of(groups, rng if shuffle else None)


def depth_text(depths, c=2, seed=5, metric_flat=0):
    """One site per depth, site after site; metric_flat: that many constant rows (flat under correlation) in front of every site."""
    rng = np.random.default_rng([seed, len(depths)])
    groups = []
    for s, n in enumerate(depths):
        X = np.vstack([np.full((metric_flat, c), 1.25), gaussian(rng, n, c, 1.0, decimals=3)])
        groups.append(site_lines('chrD', 1000 + 3 * s, '+', X, 'd%d' % s))
    return text_of(groups)


def write(tmp_path, text, name='reads.diffs.6'):
    p = str(tmp_path / name)
    open(p, 'wb').write(text)
    return p


# ---- the brute force ----
def brute_vectors(X, metric):
    """[(row index, vector)] of the usable rows, scalar Python arithmetic in the stated order."""
    out = []
    for i, v in enumerate(X):
        v = [float(x) for x in v]
        c = len(v)
        if metric == 'euclidean':
            out.append((i, v))
            continue
        m = v[0]
        for k in range(1, c):
            m = m + v[k]
        m = m / c
        w = [x - m for x in v]
        q = w[0] * w[0]
        for k in range(1, c):
            q = q + w[k] * w[k]
        if q == 0.0 or math.isinf(q) or math.isnan(q):
            continue
        s = math.sqrt(q)
        out.append((i, [x / s for x in w]))
    return out


def brute_distance(a, b, metric):
    if metric == 'euclidean':
        e = a[0] - b[0]
        acc = e * e
        for k in range(1, len(a)):
            e = a[k] - b[k]
            acc = acc + e * e
        return math.sqrt(acc)
    acc = a[0] * b[0]
    for k in range(1, len(a)):
        acc = acc + a[k] * b[k]
    return max(0.0, 1.0 - acc)


def brute_split(X, metric='correlation'):
    """-> None (fewer than 2 usable rows) or (usable row indices, labels 1 / 2 of those rows, h_top, h_sub, the pair distances).
    Clusters are lists of rows; D(A, B) is the max over all pairs, computed anew for every pair of clusters in every round."""
    vec = brute_vectors(X, metric)
    n = len(vec)
    if n < 2:
        return None
    d = [[brute_distance(vec[a][1], vec[b][1], metric) for b in range(n)] for a in range(n)]
    clusters = [([i], 0.0) for i in range(n)]                         # (rows ascending, the distance of the cluster's last merge)
    while len(clusters) > 2:
        best = None
        for x in range(len(clusters)):
            for y in range(len(clusters)):
                A, B = clusters[x][0], clusters[y][0]
                if min(A) >= min(B):                                  # A is the cluster with the smaller index
                    continue
                D = max(d[a][b] for a in A for b in B)
                cand = (D, min(A), min(B))
                if best is None or cand[0] < best[0][0] or (cand[0] == best[0][0] and (cand[1] < best[0][1] or (cand[1] == best[0][1] and
                                                                                                             cand[2] < best[0][2]))):
                    best = (cand, x, y)
        (D, _, _), x, y = best
        merged = (sorted(clusters[x][0] + clusters[y][0]), D)
        clusters = [cl for k, cl in enumerate(clusters) if k not in (x, y)] + [merged]
    first, second = sorted(clusters, key=lambda cl: min(cl[0]))
    assert min(first[0]) == 0
    labels = [1 if i in first[0] else 2 for i in range(n)]
    h_top = max(d[a][b] for a in first[0] for b in second[0])
    pairs = [d[a][b] for a in range(n) for b in range(a + 1, n)]
    return [i for i, _ in vec], labels, h_top, max(first[1], second[1]), pairs


def brute_ari(cluster, meth):
    """The adjusted Rand index from the unordered pairs, counted one by one."""
    n = len(cluster)
    tp = fp = fn = tn = 0
    for a in range(n):
        for b in range(n):
            if a == b:
                continue
            same_c, same_m = cluster[a] == cluster[b], meth[a] == meth[b]
            tp += same_c and same_m
            fp += same_c and not same_m
            fn += same_m and not same_c
            tn += not same_c and not same_m
    if fn == 0 and fp == 0:
        return 1.0
    return float(2 * (tp * tn - fn * fp)) / float((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def brute_rows(text, depth=15, max_depth=256, metric='correlation', mixed=False, min_minor=0.2, min_gap=2.0):
    """(rows, bed) of the definition as bytes."""
    sites, order = {}, []
    for line in text.decode().split('\n'):
        if not line:
            continue
        f = line.split('\t')
        key = (f[0], f[2], f[5])
        if key not in sites:
            sites[key] = [f[3], [], []]
            order.append(key)
        sites[key][1].append([float(v) for v in f[4].split(',')][:-1])
        sites[key][2].append(f[6][:1] == 'm')
    rows, bed = [], []
    for key in order:
        context, values, meth = sites[key]
        got = brute_split(values[:max_depth], metric)
        if got is None or len(got[0]) < depth:
            continue
        usable, labels, h_top, h_sub, _ = got
        m = [meth[i] for i in usable]
        n1, n2 = labels.count(1), labels.count(2)
        m1 = sum(1 for l, x in zip(labels, m) if l == 1 and x)
        m2 = sum(1 for l, x in zip(labels, m) if l == 2 and x)
        ari = brute_ari(labels, m)
        chrom, pos, strand = key
        head = [chrom, pos, str(int(pos) + 1), context]
        rows.append('\t'.join(head + [strand, str(len(values)), str(min(len(values), max_depth) - len(usable)), str(n1), str(n2), str(m1), str(m2),
                                      repr(h_top), repr(h_sub), str(np.round(ari, 3))]) + '\n')
        if mixed and min(n1, n2) / (n1 + n2) >= min_minor and h_top >= min_gap * h_sub:
            bed.append('\t'.join(head + [repr(h_top), strand, str(len(values))]) + '\n')
    return ''.join(rows).encode(), ''.join(bed).encode()
