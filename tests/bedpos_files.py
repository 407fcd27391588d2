"""Small `.diffs.<k>` texts WITH a positions file for make_bed -p on the device (tests/test_gpu_bed_positions.py; the host build of
the same arithmetic: tests/test_tstat.py).  Unlike tests/bed_files.py every row has values of its own -- repr() of seeded draws --
so a column has a spread and the t-tests are defined.  Every text is bytes; an "option set" is a dict(control=, with_probs=, gff=)."""
import random

TILE = 16384                      # bytes per tile of the line-start kernels (mc_devparse.inc: KP_TILE)
SMALL = 32                        # deepest entry whose moments a single lane sums (mc_bedsum.hip: BS_SMALL)

CHROMS = ['chr1', 'chr11', 'c', 'ecoli']
POSITIONS = ['7', '007', '123', '0123', '999999999', '0', '13240']
CONTEXTS = ['GMTGGMCGTMM', 'M', 'AM', 'TTMTCMTTCTG', 'AMA', 'GMTGGACGTMM']
LABELS = ['m6A', 'A', 'm5C', 'C']
PROBS = ['0.5', '0.04', '1.0', '0.62', ' 0.3', '0.97 ', '0.0', '0.123456789']


def values(rng, n=7, centre=None, spread=1.5):
    """n comma-separated values in repr() style; column j is drawn around centre[j]."""
    centre = centre if centre is not None else [0.0] * n
    return ','.join(repr(rng.gauss(centre[j], spread)) for j in range(n))


def row(chrom, pos, context, strand, label, feats, prob='0.5', read='r0'):
    f = [chrom, read, pos, context, feats, strand, label]
    if prob is not None:
        f.append(prob)
    return '\t'.join(f)


def join(rows, trailing_newline=True):
    return ('\n'.join(rows) + ('\n' if trailing_newline and rows else '')).encode('ascii')


def listed(chrom, pos, strand, end=None):
    return '\t'.join([chrom, pos, str(int(pos) + 1) if end is None else end, strand])


def _opts(control=False, with_probs=False, gff=False):
    return dict(control=control, with_probs=with_probs, gff=gff)


PLAIN, VO, GFF, CONTROL = _opts(), _opts(with_probs=True), _opts(gff=True), _opts(control=True)
OPTION_SETS = [PLAIN, VO, GFF, CONTROL, _opts(control=True, with_probs=True), _opts(control=True, gff=True)]

SEED_BASE = 1000                  # the random files are seeds SEED_BASE .. SEED_BASE + N_RANDOM - 1 (tests/test_tstat.py: none meets a tie)
N_RANDOM = 200


def random_case(seed):
    """-> (text, positions text, options): 1-400 rows over a few sites, about half of the sites listed, with the lines a positions
    file may hold beside them (short ones, three fields, a wrong end, doubles, blanks around)."""
    rng = random.Random(seed)
    opts = dict(rng.choice(OPTION_SETS))
    n = rng.choice([1, 2, 3, 5, 17, 64, 65, 255, 256, 257, 400]) if rng.random() < 0.5 else rng.randint(1, 400)
    chroms = rng.sample(CHROMS, rng.randint(1, 3))
    positions = rng.sample(POSITIONS, rng.randint(1, 4))
    contexts = rng.sample(CONTEXTS, rng.randint(1, 3))
    nv = rng.choice([2, 3, 7, 7, 7, 9])
    centres = {}
    rows = []
    for i in range(n):
        key = (rng.choice(chroms), rng.choice(positions), rng.choice('+-'))
        centre = centres.setdefault(key, [rng.choice([0.0, 0.0, 0.4, -2.0, 5.0]) for _ in range(nv)])
        rows.append(row(key[0], key[1], rng.choice(contexts), key[2], rng.choice(LABELS), values(rng, nv, centre, rng.choice([0.5, 1.5, 3.0])),
                        rng.choice(PROBS), read='read%d' % rng.randint(0, 9) * rng.randint(1, 3)))
    lines = []
    for c in chroms:
        for p in positions:
            for s in '+-':
                if rng.random() < 0.5:
                    lines.append(listed(c, p, s))
    lines += rng.sample(['ab', '', 'chr1\t7\t8', listed('chr1', '7', '+', end='9'), '  ' + listed(chroms[0], positions[0], '+') + ' \t',
                         listed(chroms[0], positions[0], '-') + '\tmore\tfields', listed('nowhere', '1', '+')], rng.randint(0, 5))
    if lines and rng.random() < 0.5:
        lines.append(rng.choice(lines))
    rng.shuffle(lines)
    return join(rows, trailing_newline=rng.random() < 0.8), join(lines, trailing_newline=rng.random() < 0.8), opts


# ---- the edge files: name -> (text, positions text, [option sets]) ----------------------------------------------------------------
def site_rows(rng, chrom, pos, strand, depth, context='AMA', nv=7, centre=None, spread=1.5, **kw):
    centre = centre if centre is not None else [0.3 * j - 0.8 for j in range(nv)]
    return [row(chrom, pos, context, strand, LABELS[i % 4], values(rng, nv, centre, spread), prob='0.%02d' % (i % 97 + 1), **kw) for i in range(depth)]


def interleaved_text(rng, depth=5000, shallow=100):
    """One site of `depth` rows interleaved with `shallow` sites of depth 1-3 -> (text, positions text)."""
    deep = site_rows(rng, 'deep', '9', '+', depth, context='TTMTCMTTCTG')
    rows, lines = [], [listed('deep', '9', '+')]
    for i, r in enumerate(deep):
        rows.append(r)
        if i % (depth // shallow) == 0:
            j = i // (depth // shallow)
            rows += site_rows(rng, 'chr1', str(j), '-', 1 + j % 3)
            lines.append(listed('chr1', str(j), '-'))
    return join(rows), join(lines)


def tile_edge_text(rng, delta, tile=TILE):
    """Rows such that a WANTED line starts at byte tile + delta; the read name of the line before takes up the slack."""
    rows, size, i = [], 0, 0
    while True:
        r = site_rows(rng, 'chr1', str(100 + i % 7), '+-'[i % 2], 1)[0]
        if size + len(r) + 1 + 400 > tile + delta:
            pad = tile + delta - size - (len(r) + 1)
            r = r.replace('\tr0\t', '\tr0' + 'x' * pad + '\t')
            rows.append(r)
            size += len(r) + 1
            assert size == tile + delta
            break
        rows.append(r)
        size += len(r) + 1
        i += 1
    rows += site_rows(rng, 'edge', '5', '-', 3)
    return join(rows), join([listed('edge', '5', '-')] + [listed('chr1', str(100 + k), s) for k in range(7) for s in '+-'])


def edge_cases():
    rng = random.Random(20240611)
    cases = {}
    base = site_rows(rng, 'chr1', '7', '+', 4) + site_rows(rng, 'chr1', '9', '-', 3) + site_rows(rng, 'chr11', '7', '+', 2)
    both = join([listed('chr1', '7', '+'), listed('chr1', '9', '-'), listed('chr11', '7', '+')])
    cases['plain'] = (join(base), both, [PLAIN, VO, GFF, CONTROL])
    # the positions file
    cases['positions_empty'] = (join(base), b'', [PLAIN, GFF])
    cases['positions_short_lines'] = (join(base), b'ab\n\n+\nabc', [PLAIN])
    cases['nothing_wanted'] = (join(base), join([listed('chr2', '7', '+'), listed('chr1', '8', '+')]), [PLAIN, VO, GFF])
    cases['listed_twice'] = (join(base), join([listed('chr1', '7', '+'), listed('chr1', '9', '-'), listed('chr1', '7', '+')]), [PLAIN, VO])
    cases['three_fields'] = (join(base), join(['chr1\t7\t8', listed('chr1', '9', '-'), 'chr11\t7\t8\t']), [PLAIN])
    cases['blanks_around'] = (join(base), join(['  ' + listed('chr1', '7', '+') + '  ', '\t' + listed('chr1', '9', '-') + '\t \t',
                                                listed('chr11', '7', '+') + '\textra\tfields', 'chr1 \t7\t8\t+']), [PLAIN, VO])
    cases['positions_no_trailing_newline'] = (join(base), join([listed('chr1', '9', '-'), listed('chr1', '7', '+')], trailing_newline=False), [PLAIN])
    # keys are texts
    texts = site_rows(rng, 'chr1', '007', '+', 3) + site_rows(rng, 'chr1', '7', '+', 3) + site_rows(rng, 'chr1', '7', '-', 2) + \
        site_rows(rng, 'chr11', '7', '+', 2) + site_rows(rng, 'chr1', '9', '+', 2)
    cases['text_keys_007'] = (join(texts), join([listed('chr1', '007', '+')]), [PLAIN])
    cases['text_keys_7'] = (join(texts), join([listed('chr1', '7', '+')]), [PLAIN, VO])
    cases['text_keys_wrong_end'] = (join(texts), join([listed('chr1', '7', '+', end='9'), listed('chr1', '9', '+', end='010'), listed('chr1', '7', '-', end='08')]), [PLAIN])
    cases['text_keys_strand'] = (join(texts), join([listed('chr1', '9', '-'), listed('chr11', '7', '-')]), [PLAIN])
    cases['text_keys_chr11'] = (join(texts), join([listed('chr11', '7', '+')]), [PLAIN, GFF])
    cases['position_999999999'] = (join(site_rows(rng, 'c', '999999999', '+', 3)), join([listed('c', '999999999', '+')]), [PLAIN])
    # depths: one, two, three, on both sides of the lane / wave cut-over, more than a workgroup of lines
    rows, lines = [], []
    for k, depth in enumerate([1, 2, 3, SMALL, SMALL + 1, 257, 64, 65]):
        rows += site_rows(rng, 'd', str(k), '+', depth)
        lines.append(listed('d', str(k), '+'))
    cases['depths'] = (join(rows), join(lines), [PLAIN, VO, CONTROL])
    shuffled = list(rows)
    random.Random(5).shuffle(shuffled)                                  # an entry's rows spread over several 256-line workgroups
    cases['depths_spread'] = (join(shuffled), join(lines), [PLAIN, VO])
    cases['two_values'] = (join(site_rows(rng, 'c', '1', '+', 5, nv=2) + site_rows(rng, 'c', '2', '+', 40, nv=2)), join([listed('c', '1', '+'), listed('c', '2', '+')]), [PLAIN])
    cases['interleaved_5000'] = interleaved_text(rng) + ([PLAIN, VO],)
    for delta in (-1, 0, 1):
        cases['tile_edge_%+d' % delta] = tile_edge_text(rng, delta) + ([PLAIN, VO],)
    # an UNWANTED row whose values nothing could read, and one without the centre M: neither is looked at
    odd = base[:2] + [row('chr2', '7', 'AMA', '+', 'A', 'nan,inf,,x'), row('chr1', '7', 'AAA', '+', 'A', 'oops')] + base[2:]
    cases['unwanted_unparseable'] = (join(odd), both, [PLAIN, VO])
    # every t negative and tiny: the largest one rounds to -0.0
    tiny = [row('z', '1', 'AMA', '+', 'A', '%s,%s,1.0' % (repr(-1e-05 + d), repr(-2e-05 - d))) for d in (-1.0, 1.0, 0.5, -0.5, 0.25, -0.25)]
    cases['minus_zero'] = (join(tiny), join([listed('z', '1', '+')]), [PLAIN])
    # exponents and signs as repr() writes them
    forms = [row('e', '1', 'AMA', '+', 'A', v) for v in ('1e-05,-2.5e-07,3.0', '1.5e-05,+2.5e-07,3.0', '-1e-05,0.0,3.0', '2e-05,1e-07,-0.0')]
    cases['repr_forms'] = (join(forms), join([listed('e', '1', '+')]), [PLAIN])
    return cases


def decline_cases():
    """name -> (text, positions text, options, reason code of include/mcaller_hip.h, 0-based line the decline names -- of the
    positions file for 13-15, of the rows' file otherwise)."""
    rng = random.Random(77)
    good = site_rows(rng, 'chr1', '7', '+', 3) + site_rows(rng, 'chr1', '9', '-', 3)
    lines = [listed('chr1', '7', '+'), listed('chr1', '9', '-')]

    def with_row(i, r):
        rows = list(good)
        rows[i] = r
        return join(rows)
    # the entry-level cases bring rows of two or three values: the rows before them hold as many, or the count would decline first
    good3 = site_rows(rng, 'chr1', '7', '+', 3, nv=3) + site_rows(rng, 'chr1', '9', '-', 3, nv=3)
    good2 = site_rows(rng, 'chr1', '7', '+', 3, nv=2) + site_rows(rng, 'chr1', '9', '-', 3, nv=2)
    feats = good[4].split('\t')[4]
    same = [row('s', '1', 'AMA', '+', 'A', '1.5,%s,2.0' % repr(0.1 * i)) for i in range(3)]
    far = [row('f', '1', 'AMA', '+', 'A', '%s,1.0' % repr(1e6 + d)) for d in (1e-9, -1e-9) * 40]
    big = [row('b', '1', 'AMA', '+', 'A', '%s,1.0' % v) for v in ('3e18', '3.000000001e18', '2.999999999e18')]
    return {
        'positions_high_byte': (join(good), join(lines) + 'chr\xe9\t1\t2\t+\n'.encode('latin1'), PLAIN, 13, 2),
        'positions_carriage_return': (join(good), join([lines[0] + '\r', lines[1]]), PLAIN, 14, 0),
        'positions_long_line': (join(good), join([lines[0], 'z' * 70000, lines[1]]), PLAIN, 15, 1),
        'value_nan': (with_row(4, good[4].replace(feats, 'nan,' + feats.split(',', 1)[1])), join(lines), PLAIN, 16, 4),
        'value_blank': (with_row(1, good[1].replace(good[1].split('\t')[4], ' 1.0,2.0,3.0,4.0,5.0,6.0,7.0')), join(lines), VO, 16, 1),
        'value_last_inf': (with_row(5, good[5].replace(good[5].split('\t')[4], '1.0,2.0,3.0,4.0,5.0,6.0,inf')), join(lines), PLAIN, 16, 5),
        'one_value': (join([row('chr1', '7', 'AMA', '+', 'A', '1.5'), row('chr1', '7', 'AMA', '+', 'A', '2.5')]), join(lines), PLAIN, 17, 0),
        'many_values': (join([row('chr1', '7', 'AMA', '+', 'A', ','.join(repr(0.5 + i + k) for k in range(65))) for i in range(2)]), join(lines), PLAIN, 18, 0),
        'value_count': (with_row(3, good[3].replace(good[3].split('\t')[4], '1.0,2.0,3.0')), join(lines), PLAIN, 19, 3),
        'zero_variance': (join(good3 + same), join(lines + [listed('s', '1', '+')]), PLAIN, 20, 6),
        'far_tail': (join(far), join([listed('f', '1', '+')]), PLAIN, 21, 0),
        'print_range': (join(big), join([listed('b', '1', '+')]), PLAIN, 22, 0),
        # t = 1 / d of the two rows 1 + d, 1 - d: 2.0005, as near a tie of np.round(., 3) as the digits allow
        'rounding_tie': (join(good2 + [row('t', '1', 'AMA', '+', 'A', '%s,1.0' % repr(1.0 + s / 2.0005)) for s in (1.0, -1.0)]),
                         join(lines + [listed('t', '1', '+')]), PLAIN, 23, 6),
        'too_deep': (join([row('w', '1', 'M', '+', 'A', '%s,1' % (i % 7)) for i in range(100002)]), join([listed('w', '1', '+')]), PLAIN, 24, 0),
    }
