"""Inputs of tests/test_xmfa_lift.py and tests/test_gpu_xmfa_lift.py: XMFA alignments, their .fai files and bed pairs, seeded or
hand-made, and a brute-force restatement of compare_genomes' coordinate map -- a Python loop over the columns and nothing else,
which shares no code with compare_genomes.xmfa_map.  The bed lines carry tests/gpu_compare_cases.py's probability lists, which
tests/test_twosample.py has shown the device to vouch for."""
import numpy as np

from tests import gpu_compare_cases as GC
from tests import twosample_cases as T

WIDTHS = (1, 7, 64, 80)
LETTERS = 'ACGTacgtNn'


# ---- texts ----
def wrap(text, width):
    return [text[i:i + width] for i in range(0, len(text), width)] or []


def xmfa_text(blocks, comment=True):
    """blocks: [[(seq, start, end, strand, gapped text, wrap width)]] -> the file's text."""
    out = ['#FormatVersion Mauve1', ''] if comment else []
    for entries in blocks:
        for seq, start, end, strand, text, width in entries:
            out.append('> %d:%d-%d %s genome%d.fasta' % (seq, start, end, strand, seq))
            out += wrap(text, width)
        out.append('=')
    return ('\n'.join(out) + '\n').encode()


def fai_text(lens, prefix):
    off, rows = 0, []
    for k, n in enumerate(lens):
        rows.append('%s%d\t%d\t%d\t60\t61\n' % (prefix, k + 1, n, off))
        off += n
    return ''.join(rows)


def contigs_of(lens, prefix):
    """[(name, first concatenated coordinate - 1, length)]"""
    out, off = [], 0
    for k, n in enumerate(lens):
        out.append(('%s%d' % (prefix, k + 1), off, n))
        off += n
    return out


# ---- the brute force ----
def brute_map(xmfa, n1, seqs=(1, 2)):
    """{g1: (g2, flip)} by a loop over the columns of every block, the first column of a g1 kept."""
    out = {}
    for block in xmfa.decode().split('\n=\n')[:-1] if xmfa.endswith(b'=\n') else []:
        entries = {}
        for line in block.split('\n'):
            if not line or line.startswith('#'):
                continue
            if line.startswith('>'):
                where, strand = line[1:].split()[:2]
                seq, span = where.split(':')
                cur = [int(span.split('-')[0]), int(span.split('-')[1]), strand, '']
                entries.setdefault(int(seq), cur)
            else:
                cur[3] += line
        if seqs[0] not in entries or seqs[1] not in entries:
            continue
        (s1, e1, st1, t1), (s2, e2, st2, t2) = entries[seqs[0]], entries[seqs[1]]
        if e1 == 0 or e2 == 0:
            continue
        assert len(t1) == len(t2)
        r1 = r2 = 0
        for c in range(len(t1)):
            a, b = t1[c] != '-', t2[c] != '-'
            if a and b:
                g1 = s1 + r1 if st1 == '+' else e1 - r1
                g2 = s2 + r2 if st2 == '+' else e2 - r2
                assert 1 <= g1 <= n1
                if g1 not in out:
                    out[g1] = (g2, int(st1 != st2))
            r1 += a
            r2 += b
    return out


def brute_arrays(xmfa, n1, seqs=(1, 2)):
    g2, flip = np.zeros(n1 + 1, dtype=np.int64), np.zeros(n1 + 1, dtype=np.uint8)
    for g1, (to, f) in brute_map(xmfa, n1, seqs).items():
        g2[g1], flip[g1] = to, f
    return g2, flip


def place(contigs, g):
    """(name, 0-based start) of the concatenated 1-based coordinate g."""
    for name, off, n in contigs:
        if off < g <= off + n:
            return name, g - off - 1
    raise AssertionError(g)


def brute_lift(key, mapping, contigs1, contigs2):
    chrom, start, _, strand = key
    for name, off, n in contigs1:
        if name == chrom:
            break
    else:
        return None
    if not start.isdigit() or int(start) >= n or strand not in '+-' or off + int(start) + 1 not in mapping:
        return None
    g2, flip = mapping[off + int(start) + 1]
    name2, start2 = place(contigs2, g2)
    return (name2, str(start2), str(start2 + 1), strand if not flip else {'+': '-', '-': '+'}[strand])


# ---- bed pairs ----
SITES = GC.small_sites()


def beds(mapping, contigs1, contigs2, want=(), rows=True):
    """(bed1, bed2) texts: bed1 lines on mapped bases (those of `want` first, then a spread of the others), each third without its
    partner in bed2; on an unmapped base, past a contig's end and on a contig no .fai knows; bed2 in another order with a line of
    its own.  Asserted: at least one bed1 line has its image in bed2 (rows=True) and at least one has no image."""
    mapped = sorted(mapping)
    spread = [mapped[i] for i in sorted(set(np.linspace(0, len(mapped) - 1, 7).astype(int).tolist()))] if mapped else []
    assert all(g in mapping for g in want), [g for g in want if g not in mapping]
    picks = list(want) + [g for g in spread if g not in want]
    l1, l2, used, n_rows, n_without = [], [], set(), 0, 0
    for i, g1 in enumerate(picks):
        x, y = SITES[i % len(SITES)]
        strand = '+-'[i & 1]
        chrom, start = place(contigs1, g1)
        l1.append(T.bed_line(chrom, start, strand, x))
        image = brute_lift((chrom, str(start), '', strand), mapping, contigs1, contigs2)
        assert image is not None
        if image not in used and (i % 3 != 2 or i < len(want)):
            used.add(image)
            l2.append(T.bed_line(image[0], int(image[1]), image[3], y))
            n_rows += 1
    total1 = contigs1[-1][1] + contigs1[-1][2]
    free = [g for g in range(1, total1 + 1) if g not in mapping]
    x, y = SITES[7]
    if free:
        chrom, start = place(contigs1, free[len(free) // 2])
        l1.append(T.bed_line(chrom, start, '+', x))
        n_without += 1
    l1.append(T.bed_line(contigs1[0][0], contigs1[0][2], '-', x))             # one past the contig's last base
    l1.append(T.bed_line('ghost', 3, '+', x))
    l1.append(T.bed_line(contigs1[-1][0], 0, '.', x))                          # a strand that is neither
    n_without += 3
    l2.append(T.bed_line('ghost', 3, '+', y))
    assert n_without >= 1 and (n_rows >= 1 or not rows)
    return ''.join(l1).encode(), ''.join(l2[::-1]).encode(), n_rows


def case(name, lens, blocks, seqs=(1, 2), want=(), rows=True, prefix2='b'):
    """lens: {seq: [contig lengths]} -> everything a test needs of one alignment."""
    xmfa = xmfa_text(blocks)
    n1 = sum(lens[seqs[0]])
    contigs1, contigs2 = contigs_of(lens[seqs[0]], 'a'), contigs_of(lens[seqs[1]], prefix2)
    mapping = brute_map(xmfa, n1, seqs)
    bed1, bed2, n_rows = beds(mapping, contigs1, contigs2, want, rows)
    return dict(name=name, xmfa=xmfa, fai1=fai_text(lens[seqs[0]], 'a'), fai2=fai_text(lens[seqs[1]], prefix2), bed1=bed1, bed2=bed2,
                seqs=seqs, n1=n1, n2=sum(lens[seqs[1]]), mapping=mapping, contigs1=contigs1, contigs2=contigs2, n_rows=n_rows)


def gapped(rng, k, cols):
    """k letters and cols - k gaps, the gaps in runs."""
    flags = [1] * k
    need = cols - k
    while need:
        run = min(need, int(rng.integers(1, 9)))
        at = int(rng.integers(0, len(flags) + 1))
        flags[at:at] = [0] * run
        need -= run
    return ''.join(LETTERS[int(rng.integers(len(LETTERS)))] if f else '-' for f in flags)


def random_case(seed):
    """Two or three genomes of 1 - 3 contigs; blocks of every strand pair with gap runs, 0-0 entries, missing genomes, the wrap widths
    of WIDTHS, different for the entries of a block; intervals of different blocks may overlap (first wins)."""
    for attempt in range(20):                                          # (a first block whose two entries share no column: once more)
        try:
            return _random_case(seed, attempt)
        except AssertionError:
            pass
    raise AssertionError(seed)


def _random_case(seed, attempt):
    rng = np.random.default_rng([seed, 77, attempt])
    n_genomes = int(rng.integers(2, 4))
    lens = {g: [int(rng.integers(8, 60)) for _ in range(int(rng.integers(1, 4)))] for g in range(1, n_genomes + 1)}
    seqs = (1, 2) if n_genomes == 2 or seed % 3 else (3, 1)
    blocks = []
    for b in range(int(rng.integers(2, 7))):
        spans = {}
        for g in lens:
            u = rng.random()
            if b > 0 and u < 0.15:
                continue                                               # the block lacks the genome
            if b > 0 and u < 0.27:
                spans[g] = (0, 0, 0)
                continue
            total = sum(lens[g])
            k = int(rng.integers(1, min(total, 45) + 1))
            start = int(rng.integers(1, total - k + 2))
            spans[g] = (start, start + k - 1, k)
        if not spans:
            continue
        strands = ['++', '+-', '-+', '--'][b % 4]
        cols = max(k for _, _, k in spans.values()) + int(rng.integers(0, 12))
        cols = max(cols, 1)
        entries = []
        for i, g in enumerate(sorted(spans)):
            start, end, k = spans[g]
            strand = strands[0] if g == seqs[0] else strands[1] if g == seqs[1] else '+-'[int(rng.integers(2))]
            entries.append((g, start, end, strand, gapped(rng, k, cols), WIDTHS[(b + i) % 4]))
        blocks.append(entries)
    return case('random-%d' % seed, lens, blocks, seqs)


def random_cases(n, first=0):
    return [random_case(first + i) for i in range(n)]


# ---- hand-made edges (the device's tile, word and workgroup edges) ----
def letters(k, at=0):
    return ''.join('ACGT'[(at + i) % 4] for i in range(k))


def flipped(blocks):
    """Both strands of every block flipped: the same columns, every rank counted from the other end."""
    other = {'+': '-', '-': '+'}
    return [[(seq, start, end, other[strand], text, width) for seq, start, end, strand, text, width in entries] for entries in blocks]


def plain_blocks(sizes, widths1, widths2, strands='++'):
    """One gapless block per size, on consecutive coordinates of both genomes."""
    blocks, at = [], 1
    for i, k in enumerate(sizes):
        blocks.append([(1, at, at + k - 1, strands[0], letters(k), widths1[i % len(widths1)]),
                       (2, at, at + k - 1, strands[1], letters(k, 1), widths2[i % len(widths2)])])
        at += k
    return blocks, at - 1


def edge_block_sets():
    """name -> (lens, blocks, want): the bed1 sites a case must hold."""
    out = {}
    blocks, total = plain_blocks([1, 63, 64, 65, 129], [80], [64])
    out['block sizes'] = ({1: [total], 2: [total]}, blocks, (1, 2, 64, 65, 128, 129, 193, 194, total))
    blocks, total = plain_blocks([130] * 5, [1, 63, 64, 65, 80], [80, 65, 64, 63, 1])
    out['line widths'] = ({1: [total], 2: [total]}, blocks, (1, 130, 131, total))
    # a gap run over the edge of a 64-column word in either entry; an entry that begins and one that ends with a gap
    t1 = letters(60) + '-' * 10 + letters(59, 2)
    t2 = '-' + letters(125, 1) + '---'
    out['gaps at word edges'] = ({1: [119], 2: [125]}, [[(1, 1, 119, '+', t1, 80), (2, 1, 125, '-', t2, 7)]], (4, 59, 60, 61, 116))
    t1 = '--' + letters(127)
    t2 = letters(126, 3) + '---'
    out['first and last column a gap'] = ({1: [127], 2: [126]}, [[(1, 1, 127, '+', t1, 64), (2, 1, 126, '+', t2, 80)]], (4, 64, 124))
    # START = 1 and END = the genome's last base; sites on the first and the last base of a contig; images on both sides of a
    # contig boundary of genome 2
    lens = {1: [40, 30, 30], 2: [50, 50]}
    out['contig edges'] = (lens, [[(1, 1, 100, '+', letters(100), 80), (2, 1, 100, '+', letters(100, 2), 64)]],
                           (1, 40, 41, 70, 71, 100, 50, 51))
    # 257 entries in one block: its lines span workgroups of the line kernels
    k = 20
    many = [(1, 1, k, '+', letters(k), 7), (2, 1, k, '-', letters(k, 1), 1)] + [(s, 0, 0, '+', '-' * k, 7) for s in range(3, 258)]
    out['257 entries'] = ({1: [k], 2: [k]}, [many], (1, k))
    return out


def edge_case(name):
    lens, blocks, want = edge_block_sets()[name]
    return case(name, lens, blocks, want=want)


def edge_cases():
    out = []
    for name, (lens, blocks, want) in sorted(edge_block_sets().items()):
        out.append(case(name, lens, blocks, want=want))
        out.append(case(name + ', strands flipped', lens, flipped(blocks), want=want))
    return out


def unpaired_case():
    """No block holds both genomes: no row."""
    lens = {1: [30], 2: [30]}
    blocks = [[(1, 1, 10, '+', letters(10), 7)], [(2, 1, 10, '+', letters(10), 7)], [(1, 11, 20, '+', letters(10), 80), (2, 0, 0, '+', '-' * 10, 80)]]
    return case('unpaired', lens, blocks, rows=False)


def identity_case(k=50):
    lens = {1: [20, k - 20], 2: [20, k - 20]}
    return case('identity', lens, [[(1, 1, k, '+', letters(k), 80), (2, 1, k, '+', letters(k), 7)]], prefix2='a')


def write(tmp_path, c, tag=''):
    """The case's five files -> dict(bed1=, bed2=, xmfa=, fai1=, fai2=) of paths."""
    paths = {}
    for key in ('bed1', 'bed2', 'xmfa', 'fai1', 'fai2'):
        p = str(tmp_path / ('%s%s.%s' % (tag, key, key[:3] if key != 'xmfa' else 'xmfa')))
        data = c[key]
        open(p, 'wb').write(data if isinstance(data, bytes) else data.encode())
        paths[key] = p
    return paths


def expected_rows(c):
    """The rows of the definition from the brute-force lift and compare_genomes.site_values (the statistics are not what is on trial)."""
    from mcaller_amd import compare_genomes as CG
    def read(text):
        sites = {}
        for line in text.decode().splitlines():
            f = line.split('\t')
            sites[(f[0], f[1], f[2], f[5])] = ((f[4], f[6]), np.asarray([float(v) for v in f[7].split(',')]))
        return sites
    s1, s2 = read(c['bed1']), read(c['bed2'])
    rows, n_unaligned = [], 0
    for key in s1:
        image = brute_lift(key, c['mapping'], c['contigs1'], c['contigs2'])
        if image is None:
            n_unaligned += 1
        elif image in s2:
            rows.append('\t'.join(list(key) + list(image) + list(s1[key][0]) + list(s2[image][0]) + CG.site_values(s1[key][1], s2[image][1])) + '\n')
    return ''.join(rows).encode(), len(rows), n_unaligned


# ---- files the definition refuses: name -> (XMFA text, the MC_CMP_DECLINE_* name, 0-based line named); both genomes are of 8 bases ----
GOOD = ['#FormatVersion Mauve1', '> 1:1-8 + a.fa', 'ACGTACGT', '> 2:1-8 - b.fa', 'ACGT', 'ACGT', '=']


def bad_xmfas():
    def text(changes=None, more=()):
        lines = list(GOOD)
        for at, line in (changes or {}).items():
            lines[at] = line
        return ('\n'.join(lines + list(more)) + '\n').encode('latin-1')
    return {
        'carriage return': (text({2: 'ACGTACGT\r'}), 'xmfa_byte', 2),
        'high byte in a comment': (text({0: '#Format\xe9'}), 'xmfa_byte', 0),
        'header without a strand': (text({1: '> 1:1-8 a.fa'}), 'xmfa_header', 1),
        'header without a blank': (text({1: '> 1:1-8+ a.fa'}), 'xmfa_header', 1),
        'header with a sign': (text({3: '> 2:-1-8 - b.fa'}), 'xmfa_header', 3),
        'start behind end': (text({1: '> 1:9-8 + a.fa'}), 'xmfa_header', 1),
        'sequence line before a header': (text(more=['ACGT', '=']), 'xmfa_header', 7),
        'digit in a sequence': (text({4: 'AC1T'}), 'xmfa_seq_byte', 4),
        'blank in a sequence': (text({2: 'ACGT ACG'}), 'xmfa_seq_byte', 2),
        'count': (text({1: '> 1:1-9 + a.fa'}), 'xmfa_count', 1),
        'letters in a 0-0 entry': (text({3: '> 2:0-0 + b.fa'}), 'xmfa_count', 3),
        'columns': (text({3: '> 2:1-7 - b.fa', 5: 'ACG'}), 'xmfa_columns', 3),
        'unclosed': (text(more=['> 1:1-2 + a.fa', 'AC']), 'xmfa_unclosed', 7),
        'beyond genome 1': (text({1: '> 1:2-9 + a.fa'}), 'xmfa_range', 1),
        'beyond genome 2': (text({3: '> 2:3-10 - b.fa'}), 'xmfa_range', 3),
    }


def device_makes_it(dev, tmp_path, c, tag=''):
    """The device's map equals the host's, and the device's rows, file to file, the host statement's bytes -> the two stats."""
    from mcaller_amd import compare_genomes as CG
    P = write(tmp_path, c, tag)
    lift = dict(xmfa_path=P['xmfa'], fai1=P['fai1'], fai2=P['fai2'], seqs=c['seqs'])
    want_g2, want_flip = CG.xmfa_map(P['xmfa'], c['n1'], c['seqs'], c['n2'])
    g2, flip, reason = dev.xmfa_map(path=P['xmfa'], n1=c['n1'], n2=c['n2'], seqs=c['seqs'])
    xs = dev.xmfa_map_last_stats()
    assert reason is None, (c['name'], reason, xs)
    assert np.array_equal(g2, want_g2) and np.array_equal(flip, want_flip), (c['name'], g2.tolist(), want_g2.tolist())
    assert xs['n_mapped'] == np.count_nonzero(want_g2) and xs['decline_reason'] == 0 and xs['decline_line'] == -1, (c['name'], xs)
    dev.xmfa_map_release()
    host_out, out = str(tmp_path / (tag + 'host.tsv')), str(tmp_path / (tag + 'out.tsv'))
    n = CG.compare_by_position(P['bed1'], P['bed2'], out=host_out, **lift)
    n_unaligned = CG.last_compare['n_unaligned']
    assert CG.compare_by_position_device(P['bed1'], P['bed2'], out=out, **lift) == n, c['name']
    assert CG.last_compare == dict(by='device', reason=None, n_sites=n, n_unaligned=n_unaligned), (c['name'], CG.last_compare)
    assert open(out, 'rb').read() == open(host_out, 'rb').read(), c['name']
    return xs, dev.bed_compare_last_stats()
