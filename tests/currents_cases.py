"""The inputs of tests/test_compare_currents.py and tests/test_gpu_compare_currents.py, and the brute force both hold the host
statement against: .diffs rows of a native sample and a control, written out and seeded."""
import numpy as np

C6 = 6                                        # value columns of an `-m A` row with k = 6 slots (the read quality comes behind them)


def row(chrom, pos, strand, values, quality=9.5, context='GATCMGATCGA', read='read1', label='A', prob=None):
    """One .diffs row: 8 fields with a probability, 7 (a --train row) without."""
    f = [chrom, read, str(pos), context, ','.join(repr(float(v)) for v in list(values) + [quality]), strand, label]
    if prob is not None:
        f.append(repr(float(prob)))
    return '\t'.join(f) + '\n'


def values(rng, n, c=C6, shift=0.0):
    """n rows of c deviations, two decimals (ties happen), column j shifted by shift / (1 + j)."""
    return np.round(rng.normal(0.0, 1.0, size=(n, c)) + shift / (1.0 + np.arange(c)), 2)


def site_lines(chrom, pos, strand, X, tag, probs=True, context='GATCMGATCGA'):
    """The rows of one site of one file, in order; every other one a 7-field row when probs is 'mixed'."""
    out = []
    for i, v in enumerate(X):
        prob = None if probs is False or (probs == 'mixed' and i % 2) else 0.25
        out.append(row(chrom, pos, strand, v, quality=8.0 + (i % 7) / 4, context=context, read='%s_%d' % (tag, i), prob=prob))
    return out


def interleave(groups, rng):
    """The lines of several sites shuffled together, each site's own lines in their order."""
    at = [0] * len(groups)
    order = rng.permutation(np.repeat(np.arange(len(groups)), [len(g) for g in groups]))
    out = []
    for g in order:
        out.append(groups[g][at[g]])
        at[g] += 1
    return out


def seeded_pair(n_sites, lo, hi, seed, c=C6, shuffle=True, planted=4):
    """n_sites shared sites of lo .. hi rows a file (every `planted`-th with a shift in the native sample), lines of the sites
    interleaved, plus a native-only and a control-only site -> (native text, control text) as bytes."""
    rng = np.random.default_rng([seed, n_sites])
    nat, con = [], []
    for s in range(n_sites):
        n1, n2 = (int(v) for v in rng.integers(lo, hi + 1, size=2))
        shift = 1.5 if planted and s % planted == 0 else 0.0
        strand = '+-'[s & 1]
        nat.append(site_lines('chr1', 100 + 5 * s, strand, values(rng, n1, c, shift), 'n%d' % s, probs='mixed'))
        con.append(site_lines('chr1', 100 + 5 * s, strand, values(rng, n2, c), 'c%d' % s))
    nat.append(site_lines('chr2', 7, '+', values(rng, hi, c), 'nx'))
    con.append(site_lines('chr3', 7, '+', values(rng, hi, c), 'cx'))
    if shuffle:
        return ''.join(interleave(nat, rng)).encode(), ''.join(interleave(con, rng)).encode()
    return ''.join(l for g in nat for l in g).encode(), ''.join(l for g in con for l in g).encode()


def depth_pair(pooled, c=2, seed=5):
    """One site per pooled size n (n1 = n // 2 rows native, the rest control), site after site."""
    rng = np.random.default_rng([seed, len(pooled)])
    nat, con = [], []
    for s, n in enumerate(pooled):
        n1 = n // 2
        nat += site_lines('chrD', 1000 + 3 * s, '+', values(rng, n1, c, 0.3), 'n%d' % s)
        con += site_lines('chrD', 1000 + 3 * s, '+', values(rng, n - n1, c), 'c%d' % s, probs=False)
    return ''.join(nat).encode(), ''.join(con).encode()


def files(tmp_path, native, control, names=('native.diffs.6', 'control.diffs.6')):
    p1, p2 = str(tmp_path / names[0]), str(tmp_path / names[1])
    open(p1, 'wb').write(native)
    open(p2, 'wb').write(control)
    return p1, p2


# ---- the brute force: plain dict loops and direct SciPy calls per column; nothing of compare_currents or compare_genomes ----
def brute_sites(native, control, depth):
    """[(key, context, x [n1, c], y [n2, c])] of the kept sites in the order of the keys' first native rows."""
    def read(text):
        sites, order = {}, []
        for line in text.decode().split('\n'):
            if not line:
                continue
            f = line.split('\t')
            key = (f[0], f[2], f[5].rstrip('\n'))
            if key not in sites:
                sites[key] = [f[3], []]
                order.append(key)
            sites[key][1].append([float(v) for v in f[4].split(',')][:-1])
        return sites, order
    nat, order = read(native)
    con, _ = read(control)
    return [(k, nat[k][0], np.asarray(nat[k][1]), np.asarray(con[k][1])) for k in order
            if k in con and len(nat[k][1]) >= depth and len(con[k][1]) >= depth]


def brute_logs(x, y):
    """t [c] and log10 p [4, c] of a site, column by column."""
    import warnings
    from scipy.stats import ks_2samp, kstwobign, mannwhitneyu, ranksums, ttest_ind
    t, logs = [], [[], [], [], []]
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for j in range(x.shape[1]):
            a, b = x[:, j].copy(), y[:, j].copy()
            tt = ttest_ind(a, b)
            t.append(tt.statistic)
            D = ks_2samp(a, b, method='asymp').statistic
            ps = [mannwhitneyu(a, b, alternative='two-sided', method='asymptotic').pvalue, ranksums(a, b).pvalue, tt.pvalue,
                  kstwobign.sf(np.sqrt(len(a) * len(b) / (len(a) + len(b))) * D)]
            for i in range(4):
                logs[i].append(np.log10(ps[i]))
    return t, logs


def brute_bh(L):
    """Benjamini-Hochberg in the log domain as its O(m^2) definition."""
    L = np.asarray(L, dtype=np.float64)
    m = np.float64(len(L))
    out = []
    for li in L:
        best = np.float64(0.0)
        for t in L:
            if t >= li:
                best = min(best, t + (np.log10(m) - np.log10(np.float64(np.count_nonzero(L <= t)))))
        out.append(best)
    return np.asarray(out)


def brute_rows(native, control, depth=15, fdr=False, by=None, threshold=2.0):
    """(rows, bed, the unrounded L [n, 4]) of the definition, as bytes."""
    rows, Ls = [], []
    for (chrom, pos, strand), context, x, y in brute_sites(native, control, depth):
        c = x.shape[1]
        t, logs = brute_logs(x, y)
        with np.errstate(all='ignore'):
            L = [np.minimum(0.0, np.min(np.asarray(col)) + float(np.log10(c))) for col in logs]
        Ls.append(L)
        rows.append([chrom, pos, str(int(pos) + 1), context, strand, str(len(x)), str(len(y))] + [str(np.round(v, 3)) for v in t] +
                    [str(np.round(0.0 - v, 3)) for v in L])
    Ls = np.asarray(Ls, dtype=np.float64).reshape(len(rows), 4)
    if fdr:
        for i in range(4):
            for f, q in zip(rows, brute_bh(Ls[:, i])):
                f.append(str(np.round(0.0 - q, 3)))
    bed = b''
    if by is not None:
        col = -4 + ('mwu', 'rs', 't', 'ks').index(by)
        bed = ''.join('\t'.join(f[:4] + [f[col], f[4], f[5]]) + '\n' for f in rows if float(f[col]) >= threshold).encode()
    return ''.join('\t'.join(f) + '\n' for f in rows).encode(), bed, Ls
