"""Inputs for make_bed --gff --vo and --ref on the device (tests/test_gff_stats.py on the CPU, tests/test_gpu_bed_gff.py on the GPU):
NumPy's summation order restated in plain Python, seeded arrays at every depth at which the order changes, `.diffs` texts whose
entries have those depths, random files, and FASTA texts for the slice rule and the reader's rules.  Every text is bytes."""
import math
import random

from tests import bed_files as B

# 1; below, on and above the 8 accumulators; around one leaf (128) and the first split; two leaves; around one buffer (8192); three buffers
N_LIST = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 137, 255, 256, 257, 8191, 8192, 8193, 16385]
N_RANDOM = 300
TILE = B.TILE


# ---- np.add.reduce over a contiguous float64 array, restated ------------------------------------------------------------------------
def pw(a, lo, m):
    if m < 8:
        r = 0.0
        for i in range(m):
            r += a[lo + i]
        return r
    if m <= 128:
        r = [a[lo + j] for j in range(8)]
        i = 8
        while i < m - m % 8:
            for j in range(8):
                r[j] += a[lo + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < m:
            res += a[lo + i]
            i += 1
        return res
    h = m // 2
    h -= h % 8
    return pw(a, lo, h) + pw(a, lo + h, m - h)


def np_sum(a):
    r = 0.0
    for c0 in range(0, len(a), 8192):
        r = r + pw(a, c0, min(8192, len(a) - c0))
    return r


def moments(p):
    """-> (mean, var with ddof = 1, se) of a list of floats, every operation NumPy's (nan where it divides 0 by 0)."""
    n = len(p)
    mean = np_sum(p) / float(n)
    ss = np_sum([(x - mean) * (x - mean) for x in p])
    var = ss / float(n - 1) if n > 1 else float('nan')
    se = math.sqrt(var) / math.sqrt(float(n)) if var == var else float('nan')
    return mean, var, se


def seeded_array(n, seed=0):
    """n uniforms in [0, 1) that went through repr() and float(), as a probability column does."""
    rng = random.Random(1000003 * seed + n)
    return [float(repr(rng.random())) for _ in range(n)]


def equal_array(n, value=0.5):
    """Equal values: 0.5 sums without rounding, so the spread is 0.0; 0.62 does not, and leaves an se of 1e-17 or so (printed with an exponent)."""
    return [value] * n


def variances(count=100000, seed=7):
    """-> (var, n) lists: uniform variances over many binades, and doubles within 2 ulp of a perfect square."""
    rng = random.Random(seed)
    var, n = [], []
    for i in range(count):
        if i % 2:
            v = rng.random() * 10.0 ** rng.randint(-12, 6)
        else:
            k = float(rng.randint(1, 1 << 26)) * 2.0 ** rng.randint(-30, 4)
            v = k * k                                                  # exact: k has 26 bits
            for _ in range(abs(i // 2 % 5 - 2)):
                v = math.nextafter(v, math.inf if i // 2 % 5 > 2 else 0.0)
        var.append(v)
        n.append(float(rng.choice([2, 3, 4, 9, 15, 16, 100, 4096]) if i % 3 else rng.randint(2, 100000)))
    return var, n


# ---- `.diffs` texts ---------------------------------------------------------------------------------------------------------------
def _prob(rng):
    return rng.choice(B.PROBS) if rng.random() < 0.3 else repr(rng.random())


def depth_file(seed=5):
    """One entry per depth of N_LIST, the rows of all entries interleaved (the bucket order decides the sums); entry i is
    methylated in about 0.3 or 0.7 of its rows, so --control at -t 0.5 takes about half of them."""
    rng = random.Random(seed)
    order = [i for i, n in enumerate(N_LIST) for _ in range(n)]
    rng.shuffle(order)
    rows = []
    for i in order:
        label = 'm6A' if rng.random() < (0.3, 0.7)[i % 2] else 'A'
        rows.append(B.row('chr1', str(1000 + i), 'AMA', '+-'[i % 2], label, _prob(rng), read='r%d' % rng.randint(0, 99)))
    return B.join(rows)


DEPTH_OPTIONS = [dict(depth=1, thresh=0.0, control=False), dict(depth=1, thresh=0.5, control=True)]

REF_CONTIGS = {'chr1': 200, 'chr11': 41, 'c': 30, 'ecoli': 14000}


def random_fasta(seed=11):
    """The contigs the random files name, in letters a '-' window may hold (ACGTNM, some lower-case), 60 to a line."""
    rng = random.Random(seed)
    out = []
    for name, length in sorted(REF_CONTIGS.items()):
        seq = ''.join(rng.choice('ACGTACGTACGTNMacgt') for _ in range(length))
        out.append('>%s some description\n' % name)
        out += [seq[i:i + 60] + '\n' for i in range(0, length, 60)]
    return ''.join(out).encode('ascii')


def random_case(seed):
    """-> (text, options, with_ref): bed_files.random_case's rows, every one with a probability; --gff --vo, with and without
    --control and --ref."""
    rng = random.Random(7919 * seed + 13)
    opts = dict(control=rng.random() < 0.5, with_probs=True, gff=True, depth=rng.choice([1, 1, 2, 3, 5]), thresh=rng.choice(B.THRESHOLDS))
    with_ref = rng.random() < 0.5
    n = rng.choice([1, 2, 3, 5, 17, 64, 65, 255, 256, 257, 400]) if rng.random() < 0.5 else rng.randint(1, 400)
    chroms = rng.sample(B.CHROMS, rng.randint(1, 3))
    positions = rng.sample(B.POSITIONS, rng.randint(1, 4))
    contexts = rng.sample(B.CONTEXTS, rng.randint(1, 4))
    rows = []
    for _ in range(n):
        rows.append(B.row(rng.choice(chroms), rng.choice(positions), rng.choice(contexts), rng.choice(B.STRANDS), rng.choice(B.LABELS),
                          _prob(rng), read='read%d' % rng.randint(0, 9) * rng.randint(1, 3)))
    return B.join(rows, trailing_newline=rng.random() < 0.8), opts, with_ref


# ---- --ref: one `.diffs` text, many FASTA texts -----------------------------------------------------------------------------------
REF_L = 100


def _seq(length, seed, letters='ACGTNM'):
    rng = random.Random(seed)
    return ''.join(rng.choice(letters) for _ in range(length))


SEQS = {'ctg': _seq(REF_L, 1), 'c30': _seq(30, 2), 'c41': _seq(41, 3)}


def ref_rows(contigs=None):
    """Rows at every position at which the slice rule changes, both strands, two rows an entry."""
    want = {'ctg': [0, 5, 19, 20, 21, REF_L - 21, REF_L - 20, REF_L - 1, REF_L, 999999999],
            'c30': [0, 5, 9, 10, 11, 19, 20, 21, 29, 30, 31, 50], 'c41': [0, 5, 19, 20, 21, 40, 41, 42, 61, 62]}
    rows = []
    for name in contigs or sorted(want):
        for p in want[name]:
            for strand in '+-':
                rows += [B.row(name, str(p), 'AMA', strand, 'm6A', '0.9'), B.row(name, str(p), 'AMA', strand, 'A', '0.25')]
    return B.join(rows)


def fasta(records, width=60, before='', blank_after=None):
    """records: [(title, sequence)]; width None: the whole sequence on one line; blank_after: an empty line behind that line of
    every record."""
    out = [before]
    for title, seq in records:
        out.append('>%s\n' % title)
        lines = [seq[i:i + width] for i in range(0, len(seq), width)] if width else [seq]
        for j, line in enumerate(lines):
            out.append(line + '\n')
            if blank_after == j:
                out.append('\n')
    return ''.join(out).encode('ascii')


def tile_fasta(delta, what):
    """A FASTA in which a title line (what = 'title') or a sequence line (what = 'seq') of a record the rows name starts at byte
    TILE + delta.  title: a record 'pad' fills the bytes before it.  seq: the rows' contig 'long' is 20000 bases, the line before
    the boundary is cut to fit; -> (fasta, diffs text)."""
    if what == 'title':
        head = '>pad\n'
        body, size = [], len(head)
        while size + 61 + 61 <= TILE + delta:
            body.append('A' * 60 + '\n')
            size += 61
        body.append('C' * (TILE + delta - size - 1) + '\n')
        text = head + ''.join(body)
        assert len(text) == TILE + delta
        return text.encode('ascii') + fasta([('ctg at the tile edge', SEQS['ctg'])]), ref_rows(['ctg'])
    seq = _seq(20000, 4, 'ACGT')
    text, at = '>long\n', 0
    while len(text) + 61 + 61 <= TILE + delta:
        text += seq[at:at + 60] + '\n'
        at += 60
    cut = TILE + delta - len(text) - 1
    text += seq[at:at + cut] + '\n'
    at += cut
    assert len(text) == TILE + delta
    edge = at
    while at < len(seq):
        text += seq[at:at + 60] + '\n'
        at += 60
    rows = []
    for p in (edge - 21, edge - 20, edge - 1, edge, edge + 1, edge + 20, edge + 21, 0, 19999, 20000):
        for strand in '+-':
            rows += [B.row('long', str(p), 'AMA', strand, 'm6A', '0.9'), B.row('long', str(p), 'AMA', strand, 'A', '0.25')]
    return text.encode('ascii'), B.join(rows)


def ref_cases():
    """name -> (fasta text, diffs text)."""
    recs = [('ctg', SEQS['ctg']), ('c30', SEQS['c30']), ('c41', SEQS['c41'])]
    rows = ref_rows()
    cases = {
        'width_60': (fasta(recs), rows),
        'width_1': (fasta(recs, width=1), rows),
        'whole_sequence': (fasta(recs, width=None), rows),
        'no_last_newline': (fasta(recs)[:-1], rows),
        'blank_line_inside': (fasta(recs, width=7, blank_after=1), rows),
        'text_before_first_record': (fasta(recs, before='; a comment, 12 * 3\nACGT\n\n'), rows),
        'title_with_description': (fasta([(t + '\tlength=%d  more words' % len(s), s) for t, s in recs]), rows),
        'blanks_before_the_id': (fasta([(' ' + t + ' x', s) for t, s in recs]), rows),
        'lower_case': (fasta([(t, s.lower()) for t, s in recs], width=11), rows),
        'repeated_id': (fasta([('ctg first', _seq(REF_L, 9)), ('c30', SEQS['c30']), ('ctg', _seq(77, 10)), ('c41', SEQS['c41']),
                               ('ctg last', SEQS['ctg'])]), rows),
        'prefix_ids': (fasta([('ct', _seq(50, 12)), ('ctgg', _seq(50, 13))] + recs), rows),
    }
    for delta in (-1, 0, 1):
        cases['title_at_tile%+d' % delta] = tile_fasta(delta, 'title')
        cases['sequence_line_at_tile%+d' % delta] = tile_fasta(delta, 'seq')
    return cases


REF_OPTIONS = [dict(gff=True, with_probs=False), dict(gff=True, with_probs=True), dict(gff=False, with_probs=False)]


def id_hash(name):
    """The 64-bit hash the device gives a FASTA id (KeyHash of csrc/mc_textdev.h: FNV-1a, then a finaliser)."""
    m, h = (1 << 64) - 1, 0xcbf29ce484222325
    for c in name.encode('ascii'):
        h = ((h ^ c) * 0x100000001b3) & m
    for mul in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        h = ((h ^ (h >> 33)) * mul) & m
    return h ^ (h >> 33)


def chained_ids_case():
    """-> (fasta text, diffs text): twelve records whose ids all have the hash of 'ctg' in the four bits MCALLER_BED_HASH_MASK=f
    leaves, so the table holds ONE probe chain; 'ctg' is the first, the sixth and the last record, each with another sequence."""
    same = [n for n in ('r%d' % i for i in range(1000)) if id_hash(n) & 15 == id_hash('ctg') & 15][:7]
    assert len(same) == 7
    recs = ([('ctg', _seq(REF_L, 9))] + [(n, _seq(50, 30 + i)) for i, n in enumerate(same[:4])] + [('ctg', _seq(77, 10)), ('c30', SEQS['c30'])] +
            [(n, _seq(50, 40 + i)) for i, n in enumerate(same[4:])] + [('c41', SEQS['c41']), ('ctg', SEQS['ctg'])])
    assert len(recs) == 12
    return fasta(recs), ref_rows()


def decline_cases():
    """name -> (diffs text, fasta text or None, options, reason code of include/mcaller_hip.h, 0-based line the decline names)."""
    good = [B.row('ctg', str(30 + i % 3), 'AMA', '+', 'm6A', '0.5') for i in range(6)]
    def with_line(i, line):
        rows = list(good)
        rows[i] = line
        return B.join(rows)
    plain = fasta([('ctg', SEQS['ctg'])])
    with_r = fasta([('ctg', SEQS['ctg'][:40] + 'R' + SEQS['ctg'][41:])])
    gv, g = dict(gff=True, with_probs=True), dict(gff=True, with_probs=False)
    return {
        'nan_probability': (with_line(4, B.row('ctg', '31', 'AMA', '+', 'A', 'nan')), None, gv, 25, 4),
        'twenty_digits': (with_line(2, B.row('ctg', '32', 'AMA', '+', 'A', '0.12345678901234567891')), None, gv, 25, 2),
        'unknown_contig': (with_line(3, B.row('other', '30', 'AMA', '+', 'm6A', '0.5')), plain, g, 32, 3),
        'r_in_a_minus_window': (with_line(5, B.row('ctg', '32', 'AMA', '-', 'm6A', '0.5')), with_r, g, 31, 5),
        'crlf_fasta': (B.join(good), plain.replace(b'\n', b'\r\n'), g, 29, 0),
        'blank_in_a_sequence_line': (B.join(good), plain.replace(b'\n', b' \n', 2), g, 30, 1),
    }
