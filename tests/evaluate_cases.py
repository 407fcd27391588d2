"""Cases of mcaller_amd.evaluate and a brute-force restatement of its definition (tests/test_evaluate.py).

The restatement shares nothing with the module but the file formats: a loop per row and per threshold for the integer tables;
for the subsampled depths it ENUMERATES every one of the C(N, d) subsets of a site's reads (N <= 10), takes the called fraction
of each as make_bed would (x / d in fp64, `>=` against j / 100) and counts -- no hypergeometric formula, no k_min."""
import itertools
from fractions import Fraction

import numpy as np

CONTEXT_M = 'GTAAGMTCCCT'
CONTEXT_A = 'GTAAGATCCCT'


def row(chrom, pos, strand, label, prob, context=CONTEXT_M, read='read1'):
    return '\t'.join([chrom, read, str(pos), context, '-0.4,1.6,7.05', strand, label, prob])


def site_rows(chrom, pos, strand, calls, probs=None, context=CONTEXT_M):
    """A site's rows: calls a list of 0 / 1 (1: called methylated); probs their printed probabilities."""
    probs = probs or ['0.9' if c else '0.1' for c in calls]
    return [row(chrom, pos, strand, 'm6A' if c else 'A', p, context, 'read%d' % i) for i, (c, p) in enumerate(zip(calls, probs))]


def build(sites, unlabelled=(), not_m=(), shuffle_seed=None):
    """sites: [(chrom, pos, strand, truth label, calls, probs or None)] -> (diffs bytes, positions bytes).  unlabelled / not_m: more
    rows (lists of row texts) that the evaluation skips.  The rows are interleaved by a seeded shuffle."""
    rows, plines = [], []
    for chrom, pos, strand, label, calls, probs in sites:
        rows += site_rows(chrom, pos, strand, calls, probs)
        plines.append('%s\t%d\t%s\t%s\t' % (chrom, pos, strand, label))       # (the testdata's lines end in a tab)
    rows += list(unlabelled) + list(not_m)
    if shuffle_seed is not None:
        np.random.RandomState(shuffle_seed).shuffle(rows)
    return ('\n'.join(rows) + '\n').encode('ascii'), ('\n'.join(plines) + '\n').encode('ascii')


def random_case(seed, n_sites=14, max_n=10, on_grid=True):
    """Sites of 1 .. max_n rows, both classes, calls correlated with the truth, unlabelled and non-M rows between them."""
    rng = np.random.RandomState(seed)
    sites = []
    for i in range(n_sites):
        n = int(rng.randint(1, max_n + 1))
        pos_site = bool(rng.rand() < 0.5)
        p = np.clip(rng.normal(0.65 if pos_site else 0.35, 0.25, n), 0, 1)
        probs = [str(np.round(v, 2)) if on_grid else repr(float(np.round(v, 3))) for v in p]
        calls = [1 if float(t) >= 0.5 else 0 for t in probs]
        sites.append(('chr%d' % (i % 2), 100 + 7 * i, '+-'[i % 2], 'm6A' if pos_site else 'A', calls, probs))
    unl = [row('chr0', 9000 + i, '+', 'm6A', '0.77') for i in range(5)]
    unl.append(row('chr0', 100, '-', 'A', '0.2'))                              # a labelled position on the other strand
    not_m = [row('chr0', 100, '+', 'A', '0.3', CONTEXT_A), row('chr1', 107, '-', 'm6A', '0.8', 'ACGT')]
    return build(sites, unl, not_m, shuffle_seed=seed)


def brute_force(diffs, positions, min_depth, depths):
    """-> (bytes, exact): the evaluation file, and every printed rate and AUC as an exact Fraction (None where nan), in order."""
    truth = {}
    for line in positions.decode('ascii').split('\n'):
        tok = line.split()
        if len(tok) > 1:
            truth[(tok[0], int(tok[1]), tok[2])] = tok[3]
    kept, order = [], []
    text = diffs.decode('ascii')
    for line in text.split('\n')[:-1] if text.endswith('\n') else text.split('\n'):
        f = line.split('\t')
        assert len(f) == 8
        if f[3][len(f[3]) // 2] != 'M':
            continue
        key = (f[0], int(f[2]), f[5])
        if key not in truth:
            continue
        if key not in order:
            order.append(key)
        kept.append((key, 1 if f[6][0] == 'm' else 0, float(f[7].strip())))
    is_pos = {k: truth[k][0] == 'm' for k in order}
    calls = {k: [c for kk, c, _ in kept if kk == k] for k in order}
    out, aucs, exact = ['#level\tdepth\tthreshold\tn_pos\tn_neg\ttp\tfp\ttpr\tfpr'], [], []

    def show(fr):
        exact.append(fr)
        return 'nan' if fr is None else str(np.round(np.float64(float(fr)), 4))

    def table(level, depth, tp, fp, P, Nn, integers):
        tpr = [Fraction(v) / P if P else None for v in tp]
        fpr = [Fraction(v) / Nn if Nn else None for v in fp]
        for j in range(101):
            counts = '%d\t%d' % (tp[j], fp[j]) if integers else '-\t-'
            out.append('%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s' % (level, depth, repr(j / 100), P, Nn, counts, show(tpr[j]), show(fpr[j])))
        area = None
        if P and Nn:
            xs, ys = fpr + [Fraction(0)], tpr + [Fraction(0)]
            area = sum((xs[j] - xs[j + 1]) * (ys[j] + ys[j + 1]) / 2 for j in range(101))
        aucs.append('auc\t%s\t%s\t%s' % (level, depth, show(area)))

    def scored(items):                                     # items: [(positive?, score)] -> the integer table's columns
        tp, fp = [], []
        for j in range(101):
            t = j / 100
            tp.append(sum(1 for p, s in items if p and s >= t))
            fp.append(sum(1 for p, s in items if not p and s >= t))
        return tp, fp, sum(1 for p, _ in items if p), sum(1 for p, _ in items if not p)

    table('read', '-', *scored([(is_pos[k], s) for k, _, s in kept]), integers=True)
    table('site', 'all', *scored([(is_pos[k], np.float64(sum(calls[k])) / np.float64(len(calls[k]))) for k in order if len(calls[k]) >= min_depth]),
          integers=True)
    for d in depths:
        e = {True: [Fraction(0)] * 101, False: [Fraction(0)] * 101}
        n = {True: 0, False: 0}
        for k in order:
            c = calls[k]
            if len(c) < d:
                continue
            assert len(c) <= 10, 'the enumeration is for small sites'
            n[is_pos[k]] += 1
            subsets = list(itertools.combinations(range(len(c)), d))
            called = [sum(c[i] for i in s) for s in subsets]
            for j in range(101):
                e[is_pos[k]][j] += Fraction(sum(1 for x in called if x / d >= j / 100), len(subsets))
        table('site', str(d), e[True], e[False], n[True], n[False], integers=False)
    return ('\n'.join(out + aucs) + '\n').encode('ascii'), exact

