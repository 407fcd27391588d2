"""Small `.diffs.<k>` texts for the device summary (tests/test_gpu_bed.py; their properties: tests/test_bed_files.py): a seeded
generator of in-scope files -- small alphabets, so that keys repeat and differ in single fields -- and the edge files.  Every text
is bytes; an "option set" is a dict(depth=, thresh=, control=, with_probs=, gff=) of what the device summarises."""
import random

TILE = 16384                      # bytes per tile of the line-start kernels (mc_devparse.inc: KP_TILE)

CHROMS = ['chr1', 'chr11', 'c', 'ecoli']
POSITIONS = ['7', '007', '123', '0123', '999999999', '0', '13240']
CONTEXTS = ['GMTGGMCGTMM', 'GMTGGACGTMM', 'M', 'AM', 'TTMTCMTTCTG', 'TTMTCMTTCTGA', 'AMA', 'MMM']
STRANDS = ['+', '-']
LABELS = ['m6A', 'A', 'm5C', 'C']
PROBS = ['0.5', '0.04', '1.0', '0.62', ' 0.3', '0.97 ', '0.0', '0.123456789']
THRESHOLDS = [0.0, 0.3, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.7, 1.0]


def row(chrom, pos, context, strand, label, prob=None, read='r0', feats='1.72,-1.48,1.64,-1.9,0.53,2.725,7.05'):
    f = [chrom, read, pos, context, feats, strand, label]
    if prob is not None:
        f.append(prob)
    return '\t'.join(f)


def join(rows, trailing_newline=True):
    return ('\n'.join(rows) + ('\n' if trailing_newline and rows else '')).encode('ascii')


def option_sets():
    """Every in-scope combination but for -d / -t."""
    return [dict(control=c, with_probs=v, gff=g) for g in (False, True) for v in (False, True) for c in (False, True) if not (g and v)]


def random_case(seed):
    """-> (text, options): 1-400 rows over a few sites, options drawn from the in-scope sets."""
    rng = random.Random(seed)
    opts = dict(rng.choice(option_sets()), depth=rng.choice([1, 1, 2, 3, 5]), thresh=rng.choice(THRESHOLDS))
    n = rng.choice([1, 2, 3, 5, 17, 64, 65, 255, 256, 257, 400]) if rng.random() < 0.5 else rng.randint(1, 400)
    chroms = rng.sample(CHROMS, rng.randint(1, 3))
    positions = rng.sample(POSITIONS, rng.randint(1, 4))
    contexts = rng.sample(CONTEXTS, rng.randint(1, 4))
    rows = []
    for i in range(n):
        eight = opts['with_probs'] or rng.random() < 0.8
        rows.append(row(rng.choice(chroms), rng.choice(positions), rng.choice(contexts), rng.choice(STRANDS), rng.choice(LABELS),
                        rng.choice(PROBS) if eight else None, read='read%d' % rng.randint(0, 9) * rng.randint(1, 3)))
    return join(rows, trailing_newline=rng.random() < 0.8), opts


def host_entries(text):
    """Keys of the counted rows in first-occurrence order, with [n_meth, depth] -- the yardstick's grouping, restated."""
    out = {}
    for line in text.decode('ascii').split('\n'):
        if not line:
            continue
        f = line.split('\t')
        if f[3][len(f[3]) // 2] != 'M':
            continue
        e = out.setdefault((f[0], f[2], f[5], f[3]), [0, 0])
        e[0] += f[6][0] == 'm'
        e[1] += 1
    return out


# ---- the edge files: name -> (text, [option sets with depth / thresh]) --------------------------------------------------------
def _opts(depth=1, thresh=0.5, control=False, with_probs=False, gff=False):
    return dict(depth=depth, thresh=thresh, control=control, with_probs=with_probs, gff=gff)


def tile_edge_text(delta, tile=TILE):
    """Rows such that one line starts at byte tile + delta (delta -1, 0, 1: one before, on, one after the tile boundary); the read
    name of the line before takes up the slack."""
    rows, size, i = [], 0, 0
    while True:
        r = row('chr1', str(100 + i % 7), 'GMTGGMCGTMM', '+-'[i % 2], LABELS[i % 4], PROBS[i % len(PROBS)].strip())
        if size + len(r) + 1 + 120 > tile + delta:
            pad = tile + delta - size - (len(r) + 1)
            r = row('chr1', str(100 + i % 7), 'GMTGGMCGTMM', '+-'[i % 2], LABELS[i % 4], PROBS[i % len(PROBS)].strip(), read='r0' + 'x' * pad)
            rows.append(r)
            size += len(r) + 1
            assert size == tile + delta
            break
        rows.append(r)
        size += len(r) + 1
        i += 1
    rows += [row('chr11', '5', 'AMA', '-', 'm6A', '0.9'), row('chr1', '100', 'GMTGGMCGTMM', '+', 'A', '0.1')]
    return join(rows), size


def hot_site_text(depth=100000, shallow=50):
    """One site of `depth` rows with ONE methylated call, among shallow sites (-t 0: the fraction 1e-05 at depth 10^5)."""
    rows = []
    for i in range(depth):
        if i % (depth // shallow) == 0:
            rows.append(row('chr1', str(1000 + i), 'AMA', '+', 'm6A' if i % 3 else 'A', '0.7'))
        rows.append(row('hot', '42', 'GMTGGMCGTMM', '-', 'm6A' if i == depth // 2 else 'A', '0.01'))
    return join(rows)


def interleaved_vo_text(depth=5000, shallow=1000):
    """--vo: one site of `depth` rows, every probability text different, interleaved with `shallow` sites of depth 1-3."""
    rows = []
    for i in range(depth):
        rows.append(row('deep', '9', 'TTMTCMTTCTG', '+', 'm6A' if i % 2 else 'A', '0.%04d' % (i + 1)))
        if i % (depth // shallow) == 0:
            j = i // (depth // shallow)
            for k in range(1 + j % 3):
                rows.append(row('chr1', str(j), 'AMA', '-', 'm6A' if k else 'A', '0.%d' % (k + 1)))
    return join(rows)


def fraction_rows(n_meth, depth, pos):
    return [row('f', str(pos), 'AMA', '+', 'm6A' if i < n_meth else 'A', '0.5') for i in range(depth)]


def edge_cases():
    cases = {}
    one = row('chr1', '13240', 'GMTGGMCGTMM', '-', 'm6A', '0.62')
    cases['empty_file'] = (b'', [_opts(), _opts(gff=True), _opts(with_probs=True)])
    cases['one_row'] = (join([one]), [_opts(), _opts(gff=True), _opts(with_probs=True), _opts(control=True)])
    cases['no_trailing_newline'] = (join([one, row('chr1', '13240', 'GMTGGMCGTMM', '-', 'A', '0.1')], trailing_newline=False),
                                    [_opts(), _opts(with_probs=True), _opts(depth=2, gff=True)])
    cases['no_centre_m'] = (join([row('chr1', str(i), 'GMTGGACGTMM', '+', 'm6A', '0.9') for i in range(300)]), [_opts(), _opts(with_probs=True)])
    for delta in (-1, 0, 1):
        cases['tile_edge_%+d' % delta] = (tile_edge_text(delta)[0], [_opts(), _opts(with_probs=True), _opts(gff=True, control=True)])
    # the text ends exactly on the tile boundary: the last newline is the tile's last byte
    t, size = tile_edge_text(0)
    cases['text_ends_on_tile'] = (t[:size], [_opts(), _opts(with_probs=True)])
    keys = [row('chr1', '123', 'AMA', '+', 'm6A', '0.9'), row('chr1', '123', 'AMA', '-', 'A', '0.1'),      # strand
            row('chr1', '123', 'AMC', '+', 'm6A', '0.8'),                                                  # context
            row('chr1', '0123', 'AMA', '+', 'A', '0.2'),                                                   # position text
            row('chr11', '123', 'AMA', '+', 'm6A', '0.7'),                                                 # chrom a prefix of another
            row('chr1', '123', 'AMA', '+', 'A', '0.3'), row('chr11', '123', 'AMA', '+', 'A', '0.4'), row('chr1', '0123', 'AMA', '+', 'm6A', '0.6')]
    cases['single_field_keys'] = (join(keys), [_opts(), _opts(with_probs=True), _opts(gff=True), _opts(control=True, thresh=0.6)])
    labels = [row('chr1', '5', 'AMA', '+', l, '0.5') for l in ('m6A', 'A', 'm5C', 'C', 'm6A')] + \
             [row('chr1', '6', 'CMC', '-', l, '0.5') for l in ('C', 'm5C', 'C')]
    cases['labels'] = (join(labels), [_opts(), _opts(with_probs=True), _opts(thresh=0.6), _opts(thresh=0.6, control=True)])
    cases['seven_fields'] = (join([row('chr1', str(i % 5), 'AMA', '+', 'm6A' if i % 3 else 'A') for i in range(40)]),
                             [_opts(), _opts(depth=8, gff=True), _opts(control=True, thresh=0.7)])
    fr = []
    for pos, (m, d) in enumerate([(0, 4), (4, 4), (1, 3), (2, 3), (1, 7)]):
        fr += fraction_rows(m, d, pos)
    cases['fractions'] = (join(fr), [_opts(thresh=0.0), _opts(thresh=0.0, gff=True), _opts(thresh=1.0 / 3.0), _opts(thresh=2.0 / 3.0, control=True),
                                     _opts(thresh=0.0, with_probs=True)])
    cases['hot_site'] = (hot_site_text(), [_opts(thresh=0.0), _opts(depth=1000, thresh=0.0, gff=True)])
    cases['interleaved_vo'] = (interleaved_vo_text(), [_opts(thresh=0.0, with_probs=True), _opts(depth=2, with_probs=True)])
    # more than 65536 lines: the deep bucket's row numbers need all four passes of the radix sort
    cases['interleaved_vo_wide'] = (interleaved_vo_text(depth=70000, shallow=1000), [_opts(thresh=0.0, with_probs=True)])
    # 256 lines that do not fit the 48 KB a workgroup stages: the parser reads them in place
    cases['long_lines'] = (join([row('chr1', str(i % 11), 'AMA', '+-'[i % 2], LABELS[i % 4], PROBS[i % 3], read='r%d' % i + 'y' * (300 + i % 7))
                                 for i in range(700)]), [_opts(), _opts(with_probs=True, depth=3), _opts(gff=True)])
    return cases


def decline_cases():
    """name -> (text, options, reason code of include/mcaller_hip.h, 0-based line the decline names)."""
    good = [row('chr1', str(i % 3), 'AMA', '+', 'm6A', '0.5') for i in range(6)]
    def with_line(i, line):
        rows = list(good)
        rows[i] = line
        return join(rows)
    return {
        'carriage_return': (with_line(2, good[2] + '\r'), _opts(), 2, 2),
        'high_byte': (join(good[:4]) + 'chr\xe9\tr0\t1\tAMA\t0.1\t+\tA\t0.5\n'.encode('latin1'), _opts(), 1, 4),
        'six_fields': (with_line(3, '\t'.join(good[3].split('\t')[:6])), _opts(), 3, 3),
        'empty_line': (with_line(1, ''), _opts(), 3, 1),
        'position_12a': (with_line(5, row('chr1', '12a', 'AMA', '+', 'm6A', '0.5')), _opts(), 4, 5),
        'seven_fields_vo': (with_line(0, row('chr1', '1', 'AMA', '+', 'm6A')), _opts(with_probs=True), 7, 0),
        'long_line': (with_line(4, row('chr1', '1', 'AMA', '+', 'm6A', '0.5', read='z' * 70000)), _opts(), 8, 4),
        'last_byte_line': (join(good) + b'x', _opts(), 3, 6),          # a line that starts on the last byte of the text
    }
