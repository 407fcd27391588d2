"""The brute force behind tests/test_fisher_bh.py and tests/test_gpu_compare_fdr.py: Fisher's exact test in fractions.Fraction term by
term, Benjamini-Hochberg as its O(m^2) definition, and the seeded tables, columns and BED files both tests share."""
from fractions import Fraction
from math import comb

import numpy as np

FACTOR = Fraction(1.0 + 1e-7)                 # R's factor: the fp64 number
FAR_TAIL = -250.0


def masses(K1, n1, K2, n2):
    """(lo, [P(x) C(N, d) for x in lo .. hi]) as Fractions, every term from its two binomial coefficients."""
    N, K, d = n1 + n2, K1 + K2, n1
    lo, hi = max(0, d - (N - K)), min(K, d)
    return lo, [Fraction(comb(K, x) * comb(N - K, d - x)) for x in range(lo, hi + 1)]


def masses_walked(K1, n1, K2, n2):
    """The same from the first term by the ratio of neighbours, in Fractions (deep tables: 8192 binomials of 8192 are slow)."""
    N, K, d = n1 + n2, K1 + K2, n1
    lo, hi = max(0, d - (N - K)), min(K, d)
    out = [Fraction(comb(K, lo) * comb(N - K, d - lo))]
    for x in range(lo, hi):
        out.append(out[-1] * Fraction((K - x) * (d - x), (x + 1) * (N - K - d + x + 1)))
    return lo, out


def fisher_p(K1, n1, K2, n2, walked=False):
    """The exact two-sided p, and the mass ratio P(x) / P(K1) that lies nearest to the factor (as a Fraction)."""
    lo, w = (masses_walked if walked else masses)(K1, n1, K2, n2)
    obs = w[K1 - lo]
    p = sum(v for v in w if v <= obs * FACTOR) / sum(w)
    nearest = min((v / obs for v in w), key=lambda r: abs(r - FACTOR))
    return p, nearest


def log10_exact(p):
    """The fp64 number nearest to log10 of a Fraction (mpmath at 60 digits)."""
    import mpmath
    with mpmath.workdps(60):
        return float(mpmath.log10(mpmath.mpf(p.numerator) / mpmath.mpf(p.denominator)))


def small_tables(top=12):
    """Every table with 1 <= n1, n2 <= top: sum over n1, n2 of (n1 + 1)(n2 + 1) = 8100 of them at 12."""
    return [(K1, n1, K2, n2) for n1 in range(1, top + 1) for n2 in range(1, top + 1) for K1 in range(n1 + 1) for K2 in range(n2 + 1)]


def seeded_tables(seed=31):
    """About 300 tables with pooled sizes up to 8192 -> [(name, K1, n1, K2, n2)]: random ones of every depth, lo > 0, K = 0, K = N,
    n1 = n2 with mirrored counts (P(K1) = P(K - K1): an exact selection tie), the deepest sizes the device ranks, and tables beyond
    the far tail."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(200):
        n1, n2 = (int(v) for v in rng.integers(1, [40, 300, 2000][i % 3], size=2))
        f1, f2 = rng.random(2) if i % 2 else (rng.random(),) * 2
        out.append(('random', int(rng.binomial(n1, f1)), n1, int(rng.binomial(n2, f2)), n2))
    for i in range(30):                                                   # K1 + K2 > n2: the range starts above 0
        n1, n2 = (int(v) for v in rng.integers(5, 400, size=2))
        K2 = n2 - int(rng.integers(0, 3))
        out.append(('lo > 0', int(rng.integers(max(1, n2 - K2 + 1), n1 + 1)), n1, K2, n2))
    for i in range(10):
        n1, n2 = (int(v) for v in rng.integers(1, 3000, size=2))
        out += [('K = 0', 0, n1, 0, n2), ('K = N', n1, n1, n2, n2)]
    for i in range(30):
        n = int(rng.integers(2, [30, 500, 4096][i % 3] + 1))
        a, b = (int(v) for v in rng.integers(0, n + 1, size=2))
        out += [('mirrored', a, n, b, n), ('mirrored', b, n, a, n)]
    for n1, n2 in [(4000, 4191), (4000, 4192), (4096, 4096)]:
        f = rng.random()
        out.append(('deep', int(rng.binomial(n1, f)), n1, int(rng.binomial(n2, min(1.0, f + 0.02))), n2))
    out += [('far tail', 4000, 4000, 0, 4192), ('far tail', 900, 1000, 100, 1000), ('far tail', 0, 2000, 2000, 2000)]
    return out


def bh_brute(L):
    """Q_i = min(0, min over t >= L_i of t + (log10 m - log10 #{k : L_k <= t})), t over the column's values; NaN rows stay NaN."""
    L = np.asarray(L, dtype=np.float64)
    vals = L[~np.isnan(L)]
    m = np.float64(len(vals))
    Q = np.full(len(L), np.nan)
    for i, li in enumerate(L):
        if np.isnan(li):
            continue
        best = np.float64(0.0)
        for t in vals:
            if t >= li:
                best = min(best, t + (np.log10(m) - np.log10(np.float64(np.count_nonzero(vals <= t)))))
        Q[i] = best
    return Q


def bh_columns():
    """{name: L}: ties, an all-equal column, ascending and descending input, m = 1, a NaN row."""
    rng = np.random.default_rng(41)
    base = np.log10(rng.random(60) ** 3)
    tied = np.concatenate([base[:20], base[:20], np.full(7, -1.5), np.full(3, 0.0)])
    with_nan = base.copy()
    with_nan[[3, 17, 59]] = np.nan
    return {'random': base, 'ties': tied[rng.permutation(len(tied))], 'all equal': np.full(33, -2.25), 'ascending': np.sort(base),
            'descending': np.sort(base)[::-1].copy(), 'one row': np.asarray([-3.125]), 'a NaN row': with_nan,
            'all NaN': np.full(4, np.nan), 'zeros': np.zeros(5)}


def device_column(n, seed=43):
    """A column of n log10 p for the device's sort: random magnitudes over twelve decades (every byte of the key differs somewhere),
    tie groups of 2 .. 300 rows (longer than a block of 256 wherever n allows), a few zeros and NaN rows, shuffled."""
    rng = np.random.default_rng([seed, n])
    L = -(10.0 ** rng.uniform(-9, 2.4, size=n))
    at = 0
    for size in (300, 2, 257, 5, 64):
        if at + size <= n // 2:
            L[at:at + size] = L[at]
            at += size
    if n >= 8:
        L[-1] = L[-2] = 0.0
        L[-3] = np.nan
    return L[rng.permutation(n)]


def counted_line(chrom, start, strand, K, n, values=None, frac=None):
    """A --vo BED line whose frac is the count K over n reads, as make_bed writes it: str(np.mean(labels)); the probabilities
    are independent of it."""
    if values is None:
        values = np.round(np.random.default_rng([start, n]).random(n), 2)
    if frac is None:
        frac = str(np.mean(np.asarray([1] * K + [0] * (n - K))))
    return '\t'.join([chrom, str(start), str(start + 1), 'GATC', frac, strand, str(n), ','.join(repr(float(v)) for v in values)]) + '\n'


def counted_pair(tables, first=1000, step=7, top=20):
    """tables: [(K1, n1, K2, n2)] -> (text1, text2) with one shared site a table (values drawn so that no site is degenerate)."""
    t1, t2 = [], []
    for i, (K1, n1, K2, n2) in enumerate(tables):
        pos, strand = first + i * step, '+-'[i & 1]
        t1.append(counted_line('chr1', pos, strand, K1, n1))
        t2.append(counted_line('chr1', pos, strand, K2, n2, values=np.round(np.random.default_rng([pos, n2, 2]).random(n2), 2)))
    return ''.join(t1).encode(), ''.join(t2).encode()


def recount(text):
    """A BED text with every frac rewritten as make_bed writes it: str(np.mean(p >= 0.5)) over the line's own probabilities."""
    out = []
    for line in text.decode().splitlines():
        fields = line.split('\t')
        fields[4] = str(np.mean(np.asarray([float(v) for v in fields[7].split(',')]) >= 0.5))
        out.append('\t'.join(fields) + '\n')
    return ''.join(out).encode()


def lifted_files(tmp_path):
    """An alignment with both strands flipped and its two BED files, fracs recounted -> (paths, compare_rows' keywords, rows)."""
    from tests import xmfa_cases as X
    c = dict(X.edge_cases()[1])
    c['bed1'], c['bed2'] = recount(c['bed1']), recount(c['bed2'])
    P = X.write(tmp_path, c)
    return P, dict(xmfa_path=P['xmfa'], fai1=P['fai1'], fai2=P['fai2'], seqs=c['seqs']), c['n_rows']


def planted_tables(n_sites, seed=47, top=20):
    """n_sites tables of depths 3 .. top: random, and among the first ones K1 = K2 = 0, K = N, mirrored symmetric pairs, lo > 0."""
    rng = np.random.default_rng([seed, n_sites])
    out = [(0, 7, 0, 9), (6, 6, 8, 8), (3, 10, 7, 10), (7, 10, 3, 10), (9, 10, 11, 12), (5, 5, 4, 6)][:n_sites]
    while len(out) < n_sites:
        n1, n2 = (int(v) for v in rng.integers(3, top + 1, size=2))
        out.append((int(rng.integers(0, n1 + 1)), n1, int(rng.integers(0, n2 + 1)), n2))
    return out
