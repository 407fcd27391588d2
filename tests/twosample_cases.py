"""Seeded two-sample cases for mc_twosample.h and the compare_genomes pipeline (tests/test_twosample.py, tests/test_compare_host.py,
tests/test_gpu_compare.py): the samples, the SciPy statement's text of a site, and --vo BED texts built from samples."""
import numpy as np

SIZES = [(1, 2), (2, 1), (1, 3), (3, 1), (2, 2), (3, 3), (5, 7), (20, 25), (31, 32), (32, 32), (32, 33), (40, 60), (100, 1), (1, 100),
         (500, 700), (4000, 4191), (4000, 4192)]
HOST_ONLY_SIZES = [(4000, 4193), (5000, 5000), (5000, 3)]          # more than 8192 pooled values: the device batch says TW_DEEP
KINDS = ['uniform', 'round2', 'piled', 'shift']


def sample(kind, n1, n2, seed):
    """x [n1], y [n2] in [0, 1]: 'uniform' no ties, 'round2' hundredths (ties within and across the samples), 'piled' mostly 0.0 / 0.5 /
    1.0, 'shift' y moved up by 0.15 and clipped (a pile at 1.0)."""
    rng = np.random.default_rng([seed, n1, n2, KINDS.index(kind)])
    x, y = rng.random(n1), rng.random(n2)
    if kind == 'round2':
        x, y = np.round(x, 2), np.round(y, 2)
    elif kind == 'piled':
        piles = np.asarray([0.0, 0.5, 1.0])
        x = np.where(rng.random(n1) < 0.8, piles[rng.integers(0, 3, n1)], np.round(x, 2))
        y = np.where(rng.random(n2) < 0.8, piles[rng.integers(0, 2, n2)], np.round(y, 2))
    elif kind == 'shift':
        x, y = np.round(x, 3), np.round(np.clip(y + 0.15, 0.0, 1.0), 3)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def seeded(sizes=SIZES, seed=7):
    """[(name, x, y)] over every size and kind."""
    return [('%s-%d+%d' % (kind, n1, n2), *sample(kind, n1, n2, seed)) for n1, n2 in sizes for kind in KINDS]


def far_tail():
    """Two samples apart: complete separation of 1000 against 1000 has |z| = 38.7, beyond where log10 p passes -290."""
    rng = np.random.default_rng(11)
    return np.round(rng.random(1000) * 0.2, 3), np.round(0.8 + rng.random(1000) * 0.2, 3)


# name -> (x, y, the TW_STATUS name the host build must give)
DEGENERATE = {
    'one against one': ([0.25], [0.75], 'bad_n'),
    'an empty sample': ([], [0.1, 0.2, 0.3], 'bad_n'),
    'all pooled values equal': ([0.5] * 4, [0.5] * 6, 'all_equal'),
    'two constants': ([0.25] * 5, [0.75] * 4, 'zero_var'),
    'far tail': far_tail() + ('far_tail',),
}


def statement_text(x, y):
    """The nine values of the site as compare_genomes.compare_by_position prints them (SciPy)."""
    from mcaller_amd import compare_genomes
    return compare_genomes.site_values(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))


def text_of(values):
    """The nine values of mc_twosample / mc_twosample_device as the row writer prints them: repr of each."""
    return [repr(float(v)) for v in values]


# ---- --vo BED texts ----
def number(v):
    return repr(float(v))


def bed_line(chrom, start, strand, values, end=None, context='GATC', depth=None):
    values = list(values)
    frac = repr(round(float(np.mean([v >= 0.5 for v in values])), 4)) if values else '0.0'
    return '\t'.join([chrom, str(start), str(start + 1 if end is None else end), context, frac, strand,
                      str(len(values) if depth is None else depth), ','.join(number(v) for v in values)]) + '\n'


def bed_pair(sites, chrom='chr1', first=1000, step=7):
    """sites: [(x, y)] -> (text1, text2, keys): site i at position first + i * step, strands alternating."""
    t1, t2, keys = [], [], []
    for i, (x, y) in enumerate(sites):
        strand = '+-'[i & 1]
        t1.append(bed_line(chrom, first + i * step, strand, x))
        t2.append(bed_line(chrom, first + i * step, strand, y))
        keys.append((chrom, str(first + i * step), str(first + i * step + 1), strand))
    return ''.join(t1).encode(), ''.join(t2).encode(), keys


def depth_pairs(n_sites, seed, lo=15, hi=60):
    """[(x, y)]: hundredths, depths lo .. hi, every fourth site shifted (the probe's and the GPU test's synthetic sites)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_sites):
        n1, n2 = rng.integers(lo, hi + 1, 2)
        x, y = np.round(rng.random(n1), 2), np.round(rng.random(n2), 2)
        if i % 4 == 0:
            y = np.round(np.clip(y + 0.3, 0.0, 1.0), 2)
        out.append((x, y))
    return out
