"""The inputs of tests/test_phase_edge_cases.py and tests/test_gpu_phase_edges.py: .diffs texts that put phase_reads on the GPU
(csrc/compare/mc_readphase.inc, the kr_* kernels behind Device.reads_phase) on the edges its own tests leave out -- reads of 65 ..
2048 rows whose rows arrive in no order, duplicates in a long read and at sites that are not kept, count fields of 65530 and more,
read keys and group keys that are equal in all but one field, group head lines of 256 and 65536, options and positions at the ends of
their ranges, Fisher values the device declines, lines it declines -- and `servable`: which declines the device would be allowed on a
text, decided on the CPU with the host builds only.  Every builder is seeded and returns (text, options, claims);
tests/test_phase_edge_cases.py holds each to its claims.  Built on tests/phase_cases.py; nothing here needs a GPU."""
import functools

import numpy as np

from tests import phase_cases as K

WAVE, GROUP, MAX_DEPTH = K.WAVE, K.GROUP, K.MAX_DEPTH
FE_FAR_TAIL, FE_SELECT = 2, 4                 # csrc/mc_fisher.h


def lines_of(reads, rng=None):
    return K.text_of(reads, rng).decode().splitlines(True)


def text(lines):
    return ''.join(lines).encode()


def table_reads(chrom, strand, tag, pos_a, pos_b, table):
    """Reads with a call at both positions, class after class, that make the table (n11, n10, n01, n00) of the pair."""
    reads = []
    for cls, n in enumerate(table):
        for _ in range(n):
            reads.append((chrom, '%s%d' % (tag, len(reads)), strand, [(pos_a, cls < 2), (pos_b, cls % 2 == 0)]))
    return reads


def head_line(one_text, chrom, pos, strand='+'):
    """The 0-based line of the first row of the site."""
    for no, line in enumerate(one_text.decode().splitlines()):
        f = line.split('\t')
        if (f[0], f[2], f[5]) == (chrom, str(pos), strand):
            return no
    raise KeyError((chrom, pos, strand))


# ---- servable: the declines the device is allowed on a text ----
def servable(path, opt, fdr=False, brute=None):
    """[] when the device has no reason to decline the (sound) text; else one entry per reason it would be allowed (brute: what
    phase_cases.brute returned for the text and the options, where the caller has it).  The device keeps
    a site by its ROWS (a duplicate row counts), so a duplicate declines wherever a site is kept by rows; a kept site of more than
    65535 rows, a read key of more than 2048; every written table through mc_fisher.h's host build (its status bits, the three-decimal
    tie test on the printed -log10 p as kr_finish runs it); and (fdr) the written column through mc_bh.h's."""
    from mcaller_amd import _lib
    from tests.test_phase_cases import nlp_tie
    reasons, site_rows, read_rows = [], {}, {}
    for chrom, read, pos, _, strand, _ in K.parse(path):
        site_rows[(chrom, pos, strand)] = site_rows.get((chrom, pos, strand), 0) + 1
        read_rows[(chrom, read, strand)] = read_rows.get((chrom, read, strand), 0) + 1
    kept_by_rows = [s for s, n in site_rows.items() if n >= opt['depth']]
    if not kept_by_rows:
        return reasons                                                  # nothing is written, and nothing is looked through
    reasons += [('depth', s) for s in kept_by_rows if site_rows[s] > MAX_DEPTH]
    reasons += [('read_rows', r) for r, n in read_rows.items() if n > GROUP]
    _, _, _, figures, written = brute or K.brute(path, fdr=fdr, **opt)
    if figures['n_duplicates']:
        reasons.append(('duplicate', figures['n_duplicates']))
    if not written or reasons:
        return reasons
    t = np.asarray([table for table, _ in written], dtype=np.int64)
    L, bound, status = _lib.fisher_exact(t[:, 0], t[:, 0] + t[:, 1], t[:, 2], t[:, 2] + t[:, 3])
    for table, l, b, st in zip(t.tolist(), L, bound, status):
        if st:
            reasons.append(('far_tail' if st & (1 | FE_FAR_TAIL) else 'fisher_select', tuple(table), int(st)))
        elif nlp_tie(l, b):
            reasons.append(('tie', tuple(table)))
    if fdr and not reasons:
        st = _lib.bh_adjust(L, bound)[2]
        if st:
            reasons.append(('bh_adjust', st))
    return reasons


# ---- A: long reads in any arrival order ----
LONG = (WAVE + 1, 128, 129, 1000, 1025, GROUP - 1, GROUP)
LONG_OPT = dict(depth=2, max_dist=3, min_reads=4, min_margin=1)


def long_reads(seed=5):
    """phase_cases.case_read_lengths' reads with LONG for its lengths -> (reads, the generator behind them)."""
    rng = np.random.default_rng([seed, len(LONG)])
    positions = list(range(1000, 1000 + GROUP))
    reads = K.planted_reads(rng, positions[:40], 8, 40, 40, tag='p')
    for n in LONG:
        reads.append(('chr1', 'len%d' % n, '+', [(positions[i], bool(rng.random() < 0.5)) for i in range(n)]))
    return reads, rng


@functools.lru_cache(maxsize=None)
def case_long_reads(arrival='shuffled', seed=5):
    """Reads of 65 .. 2048 rows over sites one base apart behind eight planted 40-row reads; -d 2: the 2048th position has one read
    only, so the longest read's last row stands at a site that is not kept.  arrival: 'shuffled', every row of the file at a random
    place; 'reversed', the file's lines in reverse order."""
    reads, rng = long_reads(seed)
    lines = lines_of(reads, rng) if arrival == 'shuffled' else lines_of(reads)[::-1]
    return text(lines), dict(LONG_OPT), dict(lines=6762, sites=GROUP - 1, window=3, instances=20193, lengths=LONG)


# ---- B: duplicates ----
def with_copy(lines, of, at):
    """lines with a copy of line `of` that says the opposite, inserted as line `at` (behind `of`)."""
    assert of < at <= len(lines)
    f = lines[of].rstrip('\n').split('\t')
    f[6] = 'A' if f[6] == 'm6A' else 'm6A'
    if len(f) == 8:
        f[7] = '0.25' if f[6] == 'A' else '0.75'
    return lines[:at] + ['\t'.join(f) + '\n'] + lines[at:]


def lines_with(lines, read=None, pos=None):
    return [i for i, l in enumerate(lines) if (read is None or l.split('\t')[1] == read) and (pos is None or l.split('\t')[2] == str(pos))]


@functools.lru_cache(maxsize=None)
def case_duplicate(variant):
    """-> (text, options, dict(line: the line the device names, duplicates: the host's count, ...)).
    one / two: case_long_reads('shuffled') with one (two) rows of the 1025-row read copied to a later line, opposite label;
    unkept: a duplicate at a site below -d while two sites are kept; by_duplicate: a site of d - 1 calls and one duplicate row -- d
    rows, so the device keeps it and the host does not; no_site: duplicates and no kept site."""
    if variant in ('one', 'two'):
        base, opt, _ = case_long_reads('shuffled')
        lines = base.decode().splitlines(True)
        mine = lines_with(lines, read='len1025')
        lines = with_copy(lines, mine[100], 4000)
        if variant == 'two':
            lines = with_copy(lines, mine[7], 5500)
        return text(lines), opt, dict(line=4000, duplicates=1 + (variant == 'two'), read_rows=1025 + 1 + (variant == 'two'))
    if variant == 'no_site':
        base, opt, _ = K.case_below_depth_between()
        lines = base.decode().splitlines(True)
        lines = with_copy(with_copy(lines, 3, 20), 5, 30)
        return text(lines), dict(opt, depth=100), dict(line=None, duplicates=2)
    # 18 reads at 700 and 720; `between` of them also at 710
    between = 5 if variant == 'unkept' else 14
    rng = np.random.default_rng([47, between])
    reads = []
    for r in range(18):
        calls = [(700, r & 1 == 1), (720, (r & 1 == 1) != (r % 7 == 0))]
        if r < between:
            calls.insert(1, (710, bool(rng.random() < 0.5)))
        reads.append(('chr1', 'b%d' % r, '-', calls))
    lines = lines_of(reads, rng)
    of = lines_with(lines, pos=710)[0]
    at = len(lines) - 3
    return (text(with_copy(lines, of, at)), dict(depth=15, max_dist=25, min_reads=10, min_margin=2),
            dict(line=at, duplicates=1, calls_between=between, host_sites=2, device_sites=2 + (variant == 'by_duplicate')))


# ---- C: count fields at capacity ----
DEEP_OPT = dict(depth=15, max_dist=5, min_reads=10, min_margin=1)
# (A, B, C methylated): reads; the tables of (500, 501), (500, 502), (501, 502)
DEEP_TRIPLES = [((1, 1, 1), 1), ((1, 1, 0), 1), ((0, 1, 0), 1), ((1, 0, 1), 1), ((0, 0, 1), 65529), ((0, 0, 0), 2)]
DEEP_TABLES = {'deep': [(2, 1, 1, 65531), (2, 1, 65529, 3), (1, 2, 65530, 2)],
               'deep_flipped': [(65531, 1, 1, 2), (3, 65529, 1, 2), (2, 65530, 2, 1)],
               'deep_balanced': [(16384, 16384, 16384, 16383)]}


@functools.lru_cache(maxsize=None)
def case_deep_counts(which='deep', seed=53):
    """deep: sites 500, 501 and 502 with 65535 reads over all three (DEEP_TRIPLES, the reads in a random order): n00 = 65531 in one
    written pair and n01 = 65530 in another; deep_flipped: every label flipped, n11 = 65531 and n10 = 65530; deep_balanced: two sites
    and the table (16384, 16384, 16384, 16383).  Every site has exactly 65535 rows: the cap."""
    rng = np.random.default_rng([seed, MAX_DEPTH])
    if which == 'deep_balanced':
        labels = [(cls < 2, cls % 2 == 0) for cls, n in enumerate(DEEP_TABLES[which][0]) for _ in range(n)]
    else:
        flip = which == 'deep_flipped'
        labels = [tuple(bool(m) != flip for m in triple) for triple, n in DEEP_TRIPLES for _ in range(n)]
    order = rng.permutation(len(labels))
    reads = [('chr1', 'd%d' % r, '+', [(500 + k, m) for k, m in enumerate(labels[i])]) for r, i in enumerate(order)]
    return K.text_of(reads), dict(DEEP_OPT), dict(tables=DEEP_TABLES[which], depth=MAX_DEPTH, sites=len(labels[0]))


# ---- D: keys equal in all but one field ----
# (chrom, strand, read tag): one read name on + and on -, on chrA and on chrB; ('c', '1r<k>') beside ('c1', 'r<k>') as (chrom, read);
# ('chr1', '+') beside ('chr', '1+') as (chrom, strand), with the same read names
NEAR_GROUPS = [('chrA', '+', 'n'), ('chrA', '-', 'n'), ('chrB', '+', 'n'), ('c', '+', '1r'), ('c1', '+', 'r'), ('chr1', '+', 'm'), ('chr', '1+', 'm')]


@functools.lru_cache(maxsize=None)
def case_near_keys(seed=43):
    """Seven groups of twelve reads over the same six positions seven apart, labels of their own, every row of the file at a random
    place; max_dist 20: W = 2 and 9 pairs a group, every one of them written."""
    rng = np.random.default_rng([seed, len(NEAR_GROUPS)])
    positions = [300 + 7 * i for i in range(6)]
    reads = []
    for chrom, strand, tag in NEAR_GROUPS:
        reads += K.planted_reads(rng, positions, 12, 6, 6, chrom, strand, tag=tag, every=2, noise=0.2)
    return (K.text_of(reads, rng), dict(depth=12, max_dist=20, min_reads=10, min_margin=1),
            dict(groups=len(NEAR_GROUPS), sites=6 * len(NEAR_GROUPS), reads=12 * len(NEAR_GROUPS), rows=9 * len(NEAR_GROUPS), window=2))


# ---- E: group lines beyond the low bytes ----
def filler(n, first=0):
    """n rows of a fourth chrom, a read and a site each, 10000 bases apart: no two within any max_dist used here."""
    return [K.row('chrF', 'f%d' % i, 10000 * i, '+', i % 3 == 0, seven=i % 2 == 0) for i in range(first, first + n)]


def unfilled(kept):
    """The kept sites without the filler's: those have no site behind them within max_dist, and test_phase_cases.window takes a
    time that is quadratic in the sites."""
    return [s for s in kept if s[0] != 'chrF']


@functools.lru_cache(maxsize=None)
def case_group_lines(form='full', seed=59):
    """chrA, chrB and chrC at the same positions; the first row of chrA is line 0, of chrB line 256, of chrC line 65536: head lines
    that are congruent modulo 256 and modulo 65536, so the groups' sort keys differ above bit 40 alone.
    full: 16 reads over 20 positions a group (320 rows), -d 10: chrA's first 256 rows, chrB, the rest of chrA, 64896 filler rows at
        sites of one row, chrC: 65856 lines, 60 kept sites.
    257: -d 1; chrA's 256 rows (16 reads over 16 positions) and ONE row of chrB as the last line, at chrA's second position.
    65537: -d 1; chrA's 256 rows, chrB's 256, 65024 filler rows (kept sites all), ONE row of chrC as the last line."""
    rng = np.random.default_rng([seed, len(form)])
    n_pos = 20 if form == 'full' else 16
    positions = [100 + 3 * i for i in range(n_pos)]
    group = {c: lines_of(K.planted_reads(rng, positions, 16, n_pos, n_pos, c, '+', tag='g', every=2, noise=0.2), rng) for c in ('chrA', 'chrB', 'chrC')}
    one = lambda c: [K.row(c, 'one', positions[1], '+', True)]
    if form == 'full':
        a, b, c = group['chrA'], group['chrB'], group['chrC']
        lines = a[:256] + b + a[256:] + filler(65536 - 256 - len(b) - len(a[256:])) + c
        return (text(lines), dict(depth=10, max_dist=7, min_reads=10, min_margin=2),
                dict(lines=65856, sites=60, heads={'chrA': 0, 'chrB': 256, 'chrC': 65536}, window=2))
    if form == '257':
        lines = group['chrA'] + one('chrB')
        return (text(lines), dict(depth=1, max_dist=1000, min_reads=10, min_margin=2),
                dict(lines=257, sites=17, heads={'chrA': 0, 'chrB': 256}, window=15))
    lines = group['chrA'] + group['chrB'] + filler(65536 - 512) + one('chrC')
    return (text(lines), dict(depth=1, max_dist=1000, min_reads=10, min_margin=2),
            dict(lines=65537, sites=16 + 16 + 65024 + 1, heads={'chrA': 0, 'chrB': 256, 'chrC': 65536}, window=15))


# ---- F: option and position edges ----
@functools.lru_cache(maxsize=None)
def case_max_dist(max_dist, seed=61):
    """14 reads over all of 40 sites three apart: every site behind a site is within max_dist, W = 39."""
    rng = np.random.default_rng([seed, 40])
    positions = [50 + 3 * i for i in range(40)]
    return (K.text_of(K.planted_reads(rng, positions, 14, 40, 40), rng), dict(depth=10, max_dist=max_dist, min_reads=10, min_margin=2),
            dict(window=39, sites=40))


@functools.lru_cache(maxsize=None)
def case_far_positions(seed=67):
    """Two sites, at 0 and at 999999999, with 16 reads over both."""
    rng = np.random.default_rng([seed, 2])
    return (K.text_of(K.planted_reads(rng, [0, 999999999], 16, 2, 2, every=1, noise=0.2), rng),
            dict(depth=10, max_dist=10 ** 12, min_reads=10, min_margin=2), dict(window=1, positions=['0', '999999999']))


# pos of site A -> the pair's table, B five bases behind; min_reads 10
EDGE_TABLES = {1000: (3, 2, 2, 3),        # n = 10 = min_reads
               2000: (3, 2, 2, 2),        # n = 9
               3000: (2, 0, 4, 6),        # the margin n11 + n10 = 2
               4000: (1, 0, 5, 6),        # ... = 1
               5000: (0, 0, 6, 6)}        # ... = 0: never written


@functools.lru_cache(maxsize=None)
def case_table_edges(min_margin=2, seed=71):
    rng = np.random.default_rng([seed, len(EDGE_TABLES)])
    reads = []
    for pos, table in EDGE_TABLES.items():
        reads += table_reads('chr1', '+', 'e%d_' % pos, pos, pos + 5, table)
    written = [pos for pos, t in EDGE_TABLES.items() if sum(t) >= 10 and t[0] + t[1] >= min_margin]
    return K.text_of(reads, rng), dict(depth=5, max_dist=10, min_reads=10, min_margin=min_margin), dict(written=written, window=1)


def case_no_pair():
    """phase_cases.case_shuffled under a --min_reads no table reaches (the device's option is clipped to 2^31 - 1): kept sites, reads
    rows, and no pair."""
    base, opt, _ = K.case_shuffled()
    return base, dict(opt, min_reads=2 ** 40), dict(sites=30, reads=14)


# ---- G: Fisher values the device declines ----
SERVED_TABLE, FAR_TABLE, DEEPER_TABLE = (420, 1, 1, 420), (430, 0, 0, 430), (900, 0, 0, 900)
FAR_OPT = dict(depth=15, max_dist=10, min_reads=10, min_margin=2)


@functools.lru_cache(maxsize=None)
def case_far_tail(which):
    """A served pair (sites 1000 and 1005, SERVED_TABLE) and behind it, read after read --
    served: nothing; one: a pair of FAR_TABLE at 3000 and 3005; two: that pair behind another at 5000 and 5005 (the file's order is
    not the genome's); deeper: a pair of DEEPER_TABLE.  line: the first row of site A of the first far pair of the file."""
    reads = table_reads('chr1', '+', 's', 1000, 1005, SERVED_TABLE)
    n = len(reads)
    if which == 'two':
        reads += table_reads('chr1', '+', 'x', 5000, 5005, FAR_TABLE)
    if which in ('one', 'two'):
        reads += table_reads('chr1', '+', 'f', 3000, 3005, FAR_TABLE)
    if which == 'deeper':
        reads += table_reads('chr1', '+', 'f', 3000, 3005, DEEPER_TABLE)
    return K.text_of(reads), dict(FAR_OPT), dict(line=None if which == 'served' else 2 * n, printed='246.357')


# ---- H: lines the device declines ----
def line_declines():
    """{name: (text, options, reason, the 0-based line the device names, the host's ValueError -- a piece of its words -- or None where
    the host serves the text)}: phase_cases.case_shuffled with one line changed or one line added."""
    base, opt, _ = K.case_shuffled()
    lines = base.decode().splitlines(True)
    good = K.row('chr1', 'extra', 200, '+', True)
    k = 137
    f = lines[k].rstrip('\n').split('\t')

    def changed(field, value):
        g = list(f)
        g[field] = value
        return text(lines[:k] + ['\t'.join(g) + '\n'] + lines[k + 1:])

    def added(line):
        return text(lines + [line])
    n = len(lines)
    out = {
        'high_byte': (text(lines[:k]) + lines[k].replace('GATCM', 'GATéM').encode('utf-8') + text(lines[k + 1:]), 'high_byte', k, None),
        'carriage_return': (text(lines[:k] + [lines[k][:-1] + '\r\n'] + lines[k + 1:]), 'control', k, None),
        'long_line': (added(good.replace('extra', 'r' * 70000)), 'long_line', n, None),
        'six_fields': (text(lines[:k] + ['\t'.join(f[:6]) + '\n'] + lines[k + 1:]), 'cur_fields', k, '6 tab-separated fields'),
        'nine_fields': (text(lines[:k] + ['\t'.join((f + ['0.5', 'x'])[:9]) + '\n'] + lines[k + 1:]), 'cur_fields', k, '9 tab-separated fields'),
        'no_number': (changed(4, '0.5,abc'), 'number', k, 'a value that is no number'),
        'other_count': (changed(4, '0.5,9.0,1.0'), 'cur_values', k, '3 values, 2 are expected'),
        'one_value': (text(K.row('chr1', 'r%d' % i, 200 + i % 3, '+', i & 1, values='0.5') for i in range(60)), 'cur_values', 0, 'at least 2 are needed'),
        'pos_leading_zeros': (changed(2, '00' + f[2]), 'cur_pos', k, None),
        'pos_sign': (changed(2, '+' + f[2]), 'cur_pos', k, None),
        'pos_ten_digits': (changed(2, '1234567890'), 'cur_pos', k, None),
        'pos_empty': (changed(2, ''), 'cur_pos', k, 'a position that is no integer'),
    }
    return {name: (t, dict(opt), reason, line, error) for name, (t, reason, line, error) in out.items()}


# ---- the cases the GPU tests expect the device to make: name -> builder ----
SERVED = {
    'long_shuffled': lambda: case_long_reads('shuffled'),
    'long_reversed': lambda: case_long_reads('reversed'),
    'duplicates_no_site': lambda: case_duplicate('no_site'),
    'deep': lambda: case_deep_counts('deep'),
    'deep_flipped': lambda: case_deep_counts('deep_flipped'),
    'deep_balanced': lambda: case_deep_counts('deep_balanced'),
    'near_keys': case_near_keys,
    'group_lines_full': lambda: case_group_lines('full'),
    'group_lines_257': lambda: case_group_lines('257'),
    'group_lines_65537': lambda: case_group_lines('65537'),
    'max_dist_2^31-1': lambda: case_max_dist(2 ** 31 - 1),
    'max_dist_2^31': lambda: case_max_dist(2 ** 31),
    'max_dist_10^12': lambda: case_max_dist(10 ** 12),
    'far_positions': case_far_positions,
    'table_edges_margin_2': lambda: case_table_edges(2),
    'table_edges_margin_1': lambda: case_table_edges(1),
    'no_pair': case_no_pair,
    'far_tail_served_alone': lambda: case_far_tail('served'),
}
FDR = ('deep', 'deep_flipped', 'deep_balanced', 'near_keys', 'no_pair', 'max_dist_10^12')      # the cases run with --fdr
SMALL = ('long_shuffled', 'long_reversed', 'near_keys', 'max_dist_2^31', 'far_positions', 'table_edges_margin_1', 'no_pair')
DEEP = ('deep', 'deep_flipped', 'deep_balanced')
