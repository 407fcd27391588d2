"""The inputs of tests/test_sitegroup_cases.py and tests/test_gpu_sitegroup_edges.py: .diffs texts that put the site grouping
(csrc/compare/mc_sitegroup.inc) and the two pipelines behind it (compare_currents, cluster_sites) on the edges their own tests leave
out -- unbalanced samples, one column and twenty-four, keys that differ at a field boundary only, a context per row, more than 1024
kept sites, a deep key that is not kept, numbers not spelled as repr() spells them, empty inputs, declines of single columns -- and
`servable`: which declines the device would be allowed to make on a pair of texts, decided on the CPU with the host builds only.
Seeded, built on tests/currents_cases.py and tests/cluster_cases.py; nothing here needs a GPU."""
import numpy as np

from tests import cluster_cases as KS
from tests import currents_cases as K

K_TESTS = ('mwu', 'rs', 't', 'ks')
TW_MAX_N = 8192                              # pooled values of a column the rank kernels take (mc_twosample.h)


def row_text(chrom, pos, strand, tokens, context='GATCMGATCGA', read='read1', label='A', prob=None):
    """currents_cases.row with the value tokens (the read quality last) as the strings that are written."""
    f = [chrom, read, str(pos), context, ','.join(tokens), strand, label]
    if prob is not None:
        f.append(repr(float(prob)))
    return '\t'.join(f) + '\n'


def text(lines):
    return ''.join(lines).encode()


def pair(nat_groups, con_groups, rng=None):
    """(native text, control text) of the sites' lines: site after site, or (rng) interleaved."""
    if rng is None:
        return text(l for g in nat_groups for l in g), text(l for g in con_groups for l in g)
    return text(K.interleave(nat_groups, rng)), text(K.interleave(con_groups, rng))


# ---- servable: the declines the device is allowed on a pair of texts ----
def _bits(names, st):
    return [name for name, bit in names.items() if st & bit] or ['status %d' % st]


def servable(native, control, depth, fdr=False):
    """[] when the device has no reason to decline the pair; else one entry per reason it would be allowed: every column of every kept
    site through mc_twosample's host build (its status, the bounds on the four -log10 p), the SciPy log10 p of the definition through
    mc_curcombine's host build per test, and (fdr) the four combined columns through mc_bh's."""
    from mcaller_amd import _lib
    from mcaller_amd.compare_genomes import site_values
    reasons, comb, comb_bound = [], [], []
    for key, _, x, y in K.brute_sites(native, control, depth):
        c = x.shape[1]
        if len(x) + len(y) > TW_MAX_N:
            reasons.append((key, 'depth'))
            continue
        logs, bounds, bad = [], [], False
        for j in range(c):
            xj, yj = np.ascontiguousarray(x[:, j]), np.ascontiguousarray(y[:, j])
            st, _, bound = _lib.twosample(xj, yj)
            if st:
                reasons.append((key, j, 'twosample', _bits(_lib.TW_STATUS, st)))
                bad = True
                continue
            col = []
            site_values(xj, yj, col)
            logs.append(col)
            bounds.append(bound[5:9])
        if bad:
            continue
        L, B = [], []
        for i in range(4):
            out, _, b, st = _lib.curcombine([col[i] for col in logs], [bd[i] for bd in bounds], float(np.log10(c)))
            if st:
                reasons.append((key, K_TESTS[i], 'curcombine', _bits(_lib.CC_STATUS, st)))
            L.append(out)
            B.append(b)
        comb.append(L)
        comb_bound.append(B)
    if fdr and comb and not reasons:
        comb, comb_bound = np.asarray(comb), np.asarray(comb_bound)
        for i in range(4):
            st = _lib.bh_adjust(comb[:, i], comb_bound[:, i])[2]
            if st:
                reasons.append((K_TESTS[i], 'bh_adjust', st))
    return reasons


# ---- unbalanced: one column, a sample of two rows against one of up to 8190 ----
UNBALANCED = [(2, 62), (62, 2), (2, 63), (63, 2), (510, 2), (2, 511), (2, 8190), (8190, 2)]


def unbalanced(sizes=UNBALANCED, seed=5):
    """c = 1; one site per (n1, n2), site after site, the native sample shifted by 0.3 (as currents_cases.depth_pair)."""
    rng = np.random.default_rng([seed, len(sizes)])
    nat, con = [], []
    for s, (n1, n2) in enumerate(sizes):
        nat.append(K.site_lines('chrD', 1000 + 3 * s, '+', K.values(rng, n1, 1, 0.3), 'n%d' % s))
        con.append(K.site_lines('chrD', 1000 + 3 * s, '+', K.values(rng, n2, 1), 'c%d' % s, probs=False))
    return pair(nat, con)


# ---- wide: twenty-four columns ----
WIDE_C = 24


def wide(seed=71, n_sites=12, shift=6.0):
    """12 shared sites of 3 .. 8 rows a file, interleaved; every third has 8 + 8 rows and the native sample shifted by `shift`: D = 1
    in the first columns, the least at which a Kolmogorov-Smirnov q stays below 1 behind Bonferroni's 24; and a site in either
    file alone."""
    rng = np.random.default_rng([seed, n_sites])
    nat, con = [], []
    for s in range(n_sites):
        n1, n2 = (8, 8) if s % 3 == 0 else (int(v) for v in rng.integers(3, 9, size=2))
        nat.append(K.site_lines('chrW', 100 + 5 * s, '+-'[s & 1], K.values(rng, n1, WIDE_C, shift if s % 3 == 0 else 0.0), 'n%d' % s, probs='mixed'))
        con.append(K.site_lines('chrW', 100 + 5 * s, '+-'[s & 1], K.values(rng, n2, WIDE_C), 'c%d' % s))
    nat.append(K.site_lines('chrX', 7, '+', K.values(rng, 8, WIDE_C), 'nx'))
    con.append(K.site_lines('chrY', 7, '+', K.values(rng, 8, WIDE_C), 'cx'))
    return pair(nat, con, rng)


# ---- keys: field boundaries, the ends of pos, a context per row ----
KEYS = [('chr1', 100, '+'), ('chr1', 100, '-'), ('chr1', 1000, '+'), ('chr10', 100, '+'), ('chr1', 10, '+'), ('chr11', 0, '+'),
        ('chr', 1100, '+'), ('c', 0, '+'), ('c', 999999999, '-')]
KEY_NATIVE_ONLY, KEY_CONTROL_ONLY = ('chr1', 1001, '+'), ('chr100', 0, '+')


def row_context(site, file, i):
    """11 letters that name the site, the file (n / c) and the row"""
    return 'GATCMGAT' + chr(65 + site) + 'nc'[file] + chr(65 + i)


def keyed_lines(key, X, site, file, head7):
    """The rows of a site, each with a context of its own; head7: the first row (and every other one) has 7 fields, else 8."""
    chrom, pos, strand = key
    return [K.row(chrom, pos, strand, v, quality=8.0 + (i % 7) / 4, context=row_context(site, file, i), read='%s%d_%d' % ('nc'[file], site, i),
                  prob=None if (i % 2 == 0) == bool(head7) else 0.25) for i, v in enumerate(X)]


def keys_pair(seed=73, c=2, n=3):
    """One kept site per key of KEYS (n + n rows), a native-only and a control-only key, lines interleaved in both files."""
    rng = np.random.default_rng([seed, len(KEYS)])
    nat, con = [], []
    for s, key in enumerate(KEYS):
        nat.append(keyed_lines(key, K.values(rng, n, c, 0.5 * (s % 2)), s, 0, s % 2))
        con.append(keyed_lines(key, K.values(rng, n, c), s, 1, 0))
    nat.append(keyed_lines(KEY_NATIVE_ONLY, K.values(rng, n, c), len(KEYS), 0, 0))
    con.append(keyed_lines(KEY_CONTROL_ONLY, K.values(rng, n, c), len(KEYS) + 1, 1, 1))
    return pair(nat, con, rng)


def first_contexts(one_text):
    """{key: the context of its first row} of a text, and the keys in the order of their first rows."""
    ctx, order = {}, []
    for line in one_text.decode().splitlines():
        f = line.split('\t')
        key = (f[0], int(f[2]), f[5])
        if key not in ctx:
            ctx[key] = f[3]
            order.append(key)
    return ctx, order


# ---- many: more kept sites than one round of a 1024-wide scan ----
def many_key(s):
    return 'chr%d' % (s % 5), 10 + 3 * s, '+-'[(s // 5) & 1]


def values3(rng, n, c, shift=0.0):
    """currents_cases.values with three decimals: two samples of two rows seldom have equal means (a t of 0.0 is a tie)"""
    return np.round(rng.normal(shift, 1.0, size=(n, c)), 3)


def many_pair(n_keys=1500, seed=79, c=1):
    """n_keys keys of 2 .. 3 rows a file; every 7th has one native row (below -d 2), every 11th is absent from the control, a key
    of the control alone behind every 13th; both files shuffled as wholes."""
    rng = np.random.default_rng([seed, n_keys])
    nat, con = [], []
    for s in range(n_keys):
        key = many_key(s)
        n1, n2 = (int(v) for v in rng.integers(2, 4, size=2))
        if s % 7 == 0:
            n1 = 1
        nat += K.site_lines(*key, values3(rng, n1, c, 1.0 if s % 3 == 0 else 0.0), 'n%d' % s, probs='mixed')
        if s % 11:
            con += K.site_lines(*key, values3(rng, n2, c), 'c%d' % s)
        if s % 13 == 0:
            con += K.site_lines(key[0], key[1] + 1, key[2], values3(rng, 2, c), 'o%d' % s)
    nat = [nat[i] for i in rng.permutation(len(nat))]
    con = [con[i] for i in rng.permutation(len(con))]
    return text(nat), text(con)


def many_text(n_keys=1500, seed=83, c=2):
    """The one-file version for cluster_sites: 2 .. 3 rows a key, one row at every 7th, shuffled as a whole."""
    rng = np.random.default_rng([seed, n_keys])
    lines = []
    for s in range(n_keys):
        key = many_key(s)
        n = 1 if s % 7 == 0 else int(rng.integers(2, 4))
        lines += KS.site_lines(*key, KS.gaussian(rng, n, c, 1.0, decimals=3), 's%d' % s)
    return text(lines[i] for i in rng.permutation(len(lines)))


def keys_text(seed=89, c=2, n=3):
    """The one-file version of keys_pair for cluster_sites: the native file's lines (a context per row), c = 2."""
    return keys_pair(seed, c, n)[0]


# ---- deep_unkept / deep_kept: more rows than the depth cap at a key that is not kept ----
DEEP_NATIVE, DEEP_CONTROL_ALONE = 8200, 9000
DEEP_KEY = ('chrE', 50, '+')


def deep_pair(kept, seed=97):
    """Three ordinary sites of 3 + 3 rows, c = 1; behind the first, a key with DEEP_NATIVE native rows and one control row (kept: two,
    so it is a site at -d 2, and over the cap); a key with DEEP_CONTROL_ALONE rows in the control alone.
    -> (native, control, the 0-based native line of the deep key's first row)."""
    rng = np.random.default_rng([seed, 3])
    nat, con = [], []
    for s in range(3):
        nat.append(K.site_lines('chrE', 10 + s, '+', K.values(rng, 3, 1, 0.4), 'n%d' % s))
        con.append(K.site_lines('chrE', 10 + s, '+', K.values(rng, 3, 1), 'c%d' % s))
    deep_n = K.site_lines(*DEEP_KEY, K.values(rng, DEEP_NATIVE, 1), 'dn', probs=False)
    deep_c = K.site_lines(*DEEP_KEY, K.values(rng, 2, 1), 'dc')[:2 if kept else 1]
    alone = K.site_lines('chrE', 90, '-', K.values(rng, DEEP_CONTROL_ALONE, 1), 'da', probs=False)
    nat_groups = [nat[0], deep_n, nat[1], nat[2]]
    con_groups = [con[0], alone, con[1], deep_c, con[2]]
    native, control = pair(nat_groups, con_groups)
    return native, control, len(nat[0])


# ---- spellings: every form mc_decimal.h accepts, widths that differ inside a line ----
SPELLINGS_C = 4
# (token, the value it has to read as); the read quality takes its turn too
SPELLED = [('+1.5', 1.5), ('.5', 0.5), ('5.', 5.0), ('1e-3', 0.001), ('1E2', 100.0), ('-0.0', -0.0), ('1234567890123456789e-18', 1.2345678901234568),
           ('-.25', -0.25), ('+.75e1', 7.5), ('0.1250000000000000000', 0.125), ('-2.E-1', -0.2), ('00012.50', 12.5), ('3e+0', 3.0),
           ('0.3', 0.3), ('-17', -17.0), ('9.5', 9.5), ('+0', 0.0), ('2.2250738585072014e-3', 0.0022250738585072014)]


def spellings_pair(seed=101, n_sites=3, n=4):
    """-> (native, control, native twin, control twin): the twins carry repr() of the same values.  Every row draws
    SPELLINGS_C + 1 spellings of SPELLED without replacement, the last one for its read quality."""
    rng = np.random.default_rng([seed, n_sites])
    out = [[], [], [], []]
    for s in range(n_sites):
        for file in (0, 1):
            for i in range(n):
                picks = rng.permutation(len(SPELLED))[:SPELLINGS_C + 1]
                tokens = [SPELLED[k][0] for k in picks]
                values = [SPELLED[k][1] for k in picks]
                prob = None if i % 2 else 0.25
                out[file].append(row_text('chrS', 7 + 2 * s, '+-'[s & 1], tokens, read='s%d_%d' % (s, i), prob=prob))
                out[2 + file].append(row_text('chrS', 7 + 2 * s, '+-'[s & 1], [repr(float(v)) for v in values], read='s%d_%d' % (s, i), prob=prob))
    return tuple(text(lines) for lines in out)


# ---- empty: texts without a site ----
def empty_pairs(seed=103):
    """{name: (native, control)}: an empty text on either side and on both, no shared key, shared keys all below -d 3."""
    good_n, good_c = K.seeded_pair(3, 3, 4, seed=seed, c=2, shuffle=False)
    rng = np.random.default_rng(seed)
    other = text(l for s in range(3) for l in K.site_lines('chrO', 5 + s, '+', K.values(rng, 3, 2), 'o%d' % s))
    shallow_n = text(l for s in range(3) for l in K.site_lines('chrP', 5 + s, '+', K.values(rng, 2 + (s == 1), 2), 'n%d' % s))
    shallow_c = text(l for s in range(3) for l in K.site_lines('chrP', 5 + s, '+', K.values(rng, 3 - (s == 1), 2), 'c%d' % s))
    return {'empty native': (b'', good_c), 'empty control': (good_n, b''), 'both empty': (b'', b''), 'no shared key': (good_n, other),
            'all below depth': (shallow_n, shallow_c)}


# ---- combine_declines: a site declined by one of its columns ----
def tie_column():
    """mc_twosample's status 32 (tie alone) on its host build"""
    return [0.0, 2.0], [0.9375, 0.9375]


def print_column():
    """status 96 (unprintable and tie), reported as print"""
    return [0.1, 0.1000000000001], [0.9, 0.9]


def far_tail_column(n=40, seed=107):
    """status 4 (far_tail alone): n against n, 1000 apart with a spread of 0.01"""
    rng = np.random.default_rng([seed, n])
    return list(np.round(rng.normal(0.0, 0.01, n), 4)), list(np.round(1000.0 + rng.normal(0.0, 0.01, n), 4))


def far_tail_and_tie_column():
    """status 36 (twosample_cases.far_tail: 1000 against 1000 apart), reported as far_tail"""
    from tests import twosample_cases as T
    x, y = T.far_tail()
    return list(x), list(y)


def all_equal_column(n):
    return [0.5] * n, [0.5] * n


def ordinary_column(n1, n2, rng):
    return list(np.round(rng.normal(0.3, 1.0, n1), 3)), list(np.round(rng.normal(0.0, 1.0, n2), 3))


def site_of_columns(chrom, pos, columns, tag):
    """columns: [(x_j, y_j)] -> (native lines, control lines) of the site"""
    x = np.asarray([col[0] for col in columns], dtype=np.float64).T
    y = np.asarray([col[1] for col in columns], dtype=np.float64).T
    return K.site_lines(chrom, pos, '+', x, 'n' + tag, probs='mixed'), K.site_lines(chrom, pos, '+', y, 'c' + tag)


def declining_site(what, c, pos, rng, column=None):
    """A site of c columns whose column `column` (default: the last) is `what`, the others ordinary."""
    bad = {'tie': tie_column, 'print': print_column, 'far_tail': far_tail_column, 'far_tail_and_tie': far_tail_and_tie_column}[what]()
    n1, n2 = len(bad[0]), len(bad[1])
    column = c - 1 if column is None else column
    return site_of_columns('chrC', pos, [bad if j == column else ordinary_column(n1, n2, rng) for j in range(c)], what)


def good_site(c, pos, rng, n=4):
    return site_of_columns('chrC', pos, [ordinary_column(n, n, rng) for _ in range(c)], 'good%d' % pos)


def combine_declines(seed=109):
    """{name: (native, control, depth, the reason the device gives, the 0-based native line it names)}.  Every pair starts with a good
    site of four rows a file, so the declining site's head is native line 4."""
    rng = np.random.default_rng(seed)
    out = {}
    for what, reason in (('tie', 'tie'), ('print', 'print'), ('far_tail', 'far_tail'), ('far_tail_and_tie', 'far_tail')):
        g, d = good_site(3, 10, rng), declining_site(what, 3, 20, rng)
        out['column 2 is ' + what] = pair([g[0], d[0]], [g[1], d[1]]) + (2, reason, 4)
    # column 0 all equal, column 1 far_tail: cu_tw_reason names all_equal
    ft = far_tail_column()
    g, d = good_site(2, 10, rng), site_of_columns('chrC', 20, [all_equal_column(len(ft[0])), ft], 'ae')
    out['all_equal before far_tail'] = pair([g[0], d[0]], [g[1], d[1]]) + (2, 'all_equal', 4)
    # two declining sites: the smaller head line names the reason
    g = good_site(3, 10, rng)
    tie, far = declining_site('tie', 3, 20, rng), declining_site('far_tail', 3, 30, rng)
    out['tie before far_tail'] = pair([g[0], tie[0], far[0]], [g[1], far[1], tie[1]]) + (2, 'tie', 4)
    out['far_tail before tie'] = pair([g[0], far[0], tie[0]], [g[1], tie[1], far[1]]) + (2, 'far_tail', 4)
    return out
