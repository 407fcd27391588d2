"""The inputs of tests/test_gpu_compare.py: where the kernels of csrc/compare/mc_bedcompare.hip can go wrong.  Every site of a case
that demands the device's own bytes comes from device_site_sets(), which tests/test_twosample.py holds against the host build of
mc_twosample.h: none of them is degenerate or on a rounding tie."""
import numpy as np

from tests import twosample_cases as T

EDGE_SIZES = [(2, 1), (31, 32), (32, 32), (32, 33), (256, 256), (256, 257), (4000, 4191), (4000, 4192)]      # pooled 3, 63, 64, 65, 512, 513, 8191, 8192
EDGE_SEED = 5
STRADDLE_SITES = 1100             # bed1 lines beyond kc_parse's 256 a workgroup and kp_scan's 1024 a round, text beyond a 16 KB tile


def exact_tie_site():
    """36 against 27 values whose rank-sum z is EXACTLY 0.1875 (R1 - n1 (n + 1) / 2 = 13.5, n1 n2 (n + 1) / 12 = 72^2): a rounding tie
    of np.round(., 3) that both sides must round half-way to even alike, and pooled 63: the wave kernel."""
    ranks_x = [r for r in range(1, 64) if r <= 17 or r >= 46] + [31]           # the symmetric 36 (sum 1152) with 18 -> 31: + 13
    x = [r / 100 for r in ranks_x]
    y = [r / 100 for r in range(1, 64) if r not in ranks_x]
    y[y.index(0.18)] = 0.17                                                    # y's 18 ties with x's 17: + 0.5
    return np.asarray(x), np.asarray(y)


def equal_means_site():
    """Two samples with equal means: t is 0.0 on the host, and the device has to know it is not -0.0."""
    return np.asarray([0.1, 0.4, 0.8, 0.35, 0.6]), np.asarray([0.45, 0.45, 0.2, 0.7])


def edge_sites():
    return [T.sample(kind, n1, n2, EDGE_SEED) for n1, n2 in EDGE_SIZES for kind in ('round2', 'shift')] + [exact_tie_site(), equal_means_site()]


def straddle_sites():
    return T.depth_pairs(STRADDLE_SITES, seed=21, lo=3, hi=12)


def key_sites():
    return T.depth_pairs(8, seed=22)


def small_sites():
    return T.depth_pairs(40, seed=23)


def device_site_sets():
    return {'edges': edge_sites(), 'straddle': straddle_sites(), 'keys': key_sites(), 'small': small_sites()}


def straddle_pair():
    """bed1 has every site, bed2 every site but each third, and lines of its own in between and in another order: the shared sites lie
    on both sides of every tile edge of bed1."""
    sites = straddle_sites()
    l1, l2 = [], []
    for i, (x, y) in enumerate(sites):
        strand = '+-'[i & 1]
        l1.append(T.bed_line('chrA', 10 + 3 * i, strand, x))
        if i % 3 != 1:
            l2.append(T.bed_line('chrA', 10 + 3 * i, strand, y))
        if i % 5 == 0:
            l2.append(T.bed_line('chrB', 10 + 3 * i, strand, y))
    l2 = l2[::-1]
    return ''.join(l1).encode(), ''.join(l2).encode()


def key_pair():
    """Keys that differ only in strand, only in `end`, only in a trailing byte of chrom or start: eight lines a file, pairwise
    different keys, bed2 in another order and with two keys bed1 lacks."""
    s = key_sites()
    keys = [('chr1', 100, 101, '+'), ('chr1', 100, 101, '-'), ('chr1', 100, 102, '+'), ('chr1', 1000, 101, '+'), ('chr10', 100, 101, '+'),
            ('chr1', 10, 101, '+'), ('chr1', 100, 10, '+'), ('chr', 1100, 101, '+')]
    l1 = [T.bed_line(c, a, st, x, end=e) for (c, a, e, st), (x, _) in zip(keys, s)]
    l2 = [T.bed_line(c, a, st, y, end=e) for (c, a, e, st), (_, y) in zip(keys, s)]
    extra = [T.bed_line('chr1', 100, '.', s[0][1], end=101), T.bed_line('chr1', 101, '+', s[1][1], end=100)]
    return ''.join(l1).encode(), ''.join(l2[::-1] + extra).encode()


def small_pair():
    t1, t2, _ = T.bed_pair(small_sites())
    return t1, t2


def edge_pair():
    t1, t2, _ = T.bed_pair(edge_sites())
    return t1, t2


# ---- every decline reason once: name -> (text1, text2, reason name, file, 0-based line in it, the host's exception or None) ----
def declines():
    ok1, ok2, _ = T.bed_pair(T.depth_pairs(3, seed=24))
    a1, a2 = ok1.decode(), ok2.decode()
    line = lambda vals, pos=5000, chrom='chr1', strand='+': T.bed_line(chrom, pos, strand, vals)
    good = [0.1, 0.4, 0.8, 0.35]
    far_x, far_y = T.far_tail()
    cases = {
        'high_byte': (a1, a2 + line(good).replace('GATC', 'GATé'), 'high_byte', 2, 3, None),
        'control': (a1 + line(good).replace('GATC', 'GA\x01C'), a2, 'control', 1, 3, None),
        'fields_7': (a1 + 'chr1\t1\t2\tGATC\t0.5\t+\t0.1,0.2\n', a2, 'fields', 1, 3, ValueError),
        'fields_10': (a1, a2 + line(good).rstrip('\n') + '\tx\ty\n', 'fields', 2, 3, ValueError),
        'empty_key': (a1 + line(good, chrom=''), a2, 'empty', 1, 3, None),
        'empty_list': (a1, line([]) + a2, 'empty', 2, 0, ValueError),
        'long_line': (a1 + line(good).replace('GATC', 'G' * 70000), a2, 'long_line', 1, 3, None),
        'duplicate_1': (a1 + a1.splitlines(True)[1], a2, 'duplicate', 1, 3, None),
        'duplicate_2': (a1, a2 + line(good, 7000) + line(good, 7000), 'duplicate', 2, 4, None),
        'number': (a1 + line(good), a2 + line(good).replace('0.35', ' 0.35'), 'number', 2, 3, None),
        'number_nan': (a1 + line(good).replace('0.35', 'nan'), a2 + line(good), 'number', 1, 3, None),
        'nan': (a1 + line([0.25]), a2 + line([0.75]), 'nan', 1, 3, None),
        'zero_var': (a1 + line([0.25] * 3), a2 + line([0.75] * 4), 'nan', 1, 3, None),
        'all_equal': (line([0.5] * 3) + a1, a2 + line([0.5] * 4), 'all_equal', 1, 0, None),
        'far_tail': (a1 + line(far_x), a2 + line(far_y), 'far_tail', 1, 3, None),
        'print': (a1 + line([0.1, 0.1000000000001]), a2 + line([0.9]), 'print', 1, 3, None),       # t = -1e13
        'tie': (a1 + line([0.0, 2.0]), a2 + line([0.9375, 0.9375]), 'tie', 1, 3, None),              # t = 0.0625 but for the sums of squares' roundings
        'number_bed1_only': (a1 + line(good, 9000).replace('0.35', '0.3x5'), a2, 'number', 1, 3, ValueError),
        'number_bed2_only': (a1, a2 + line(good, 9001).replace('0.4,', '0.4,,'), 'number', 2, 3, ValueError),
    }
    return {k: (v[0].encode('utf-8'), v[1].encode('utf-8')) + v[2:] for k, v in cases.items()}


def deep_pair():
    """One shared site of 8193 pooled values among shallow ones."""
    x, y = T.sample('round2', 4000, 4193, 5)
    ok = T.depth_pairs(2, seed=25)
    t1, t2, _ = T.bed_pair([ok[0], (x, y), ok[1]])
    return t1, t2
