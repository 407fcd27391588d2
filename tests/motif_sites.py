"""find_motifs restated by brute force -- plain loops over strings, no code shared with mcaller_amd/find_motifs.py -- and the
inputs the CPU and GPU tests share: random genomes, site lists, the placed cases, the planted-motif genome."""
import random

COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def revcomp(s):
    return ''.join(COMP.get(ch, 'N') for ch in reversed(s))


def brute_tables(contigs, bed, control, base, shapes):
    """{(shape index, j, letters): [nGenome, nCovered, nMethylated]} by a loop over every candidate, shape and X."""
    ref = {}
    for name, seq in contigs:
        ref[name] = seq.upper()
    meth, ctl = set(bed), (None if control is None else set(control))
    tables = {}
    for name, seq in ref.items():
        for p in range(len(seq)):
            for strand in '+-':
                on_strand = seq[p] if strand == '+' else COMP.get(seq[p])
                if on_strand != base:
                    continue
                site = (name, p, strand)
                is_meth = site in meth
                is_cov = True if ctl is None else (is_meth or site in ctl)
                for si, shape in enumerate(shapes):
                    W = len(shape)
                    xs = [i for i in range(W) if shape[i] == 'X']
                    for j, o in enumerate(xs):
                        if strand == '+':
                            a, b = p - o, p - o + W
                        else:
                            a, b = p - (W - 1 - o), p + o + 1
                        if a < 0 or b > len(seq):
                            continue
                        window = seq[a:b] if strand == '+' else revcomp(seq[a:b])
                        letters = ''.join(window[x] for x in xs)
                        if any(ch not in 'ACGT' for ch in letters):
                            continue
                        t = tables.setdefault((si, j, letters), [0, 0, 0])
                        t[0] += 1
                        t[1] += is_cov
                        t[2] += is_meth
    return tables


def brute(contigs, bed, control, base='A', shapes=None, min_sites=20, min_fraction=0.5, keep_all=False, tables=None):
    """contigs: [(id, sequence as in the file)]; bed / control: lists of (chrom, start, strand) (control may be None) -> the text.
    tables: brute_tables of the same inputs, where a test selects from them more than once."""
    if tables is None:
        tables = brute_tables(contigs, bed, control, base, shapes)
    selected = {}
    for (si, j, letters), (nG, nC, nM) in tables.items():
        if nM >= min_sites and nC > 0 and nM / nC >= min_fraction:
            selected[(si, j, letters)] = (nG, nC, nM)

    def placed(si, j, letters):
        xs = [i for i in range(len(shapes[si])) if shapes[si][i] == 'X']
        return {x - xs[j]: ch for x, ch in zip(xs, letters)}
    rows = []
    for key, (nG, nC, nM) in selected.items():
        mine = placed(*key)
        redundant = False
        if not keep_all:
            for other in selected:
                theirs = placed(*other)
                if len(theirs) < len(mine) and all(mine.get(r) == ch for r, ch in theirs.items()):
                    redundant = True
        if not redundant:
            rows.append((-nM, -(nM / nC), key[0], key[1], key[2], nG, nC, nM))
    rows.sort()
    out = []
    for _, _, si, j, letters, nG, nC, nM in rows:
        spec, i = '', 0
        for ch in shapes[si]:
            if ch == 'X':
                spec += letters[i]
                i += 1
            else:
                spec += 'N'
        o = [x for x in range(len(shapes[si])) if shapes[si][x] == 'X'][j]
        out.append('%s:%d\t%d\t%d\t%d\t%r\n' % (spec, o + 1, nG, nC, nM, nM / nC))
    return ''.join(out).encode('ascii')


def default_shapes():
    return ['XXX', 'XXXX', 'XXXXX', 'XXXXXX'] + ['X' * a + '.' * g + 'X' * b for a in (3, 4) for g in (5, 6, 7, 8) for b in (3, 4)]


def fasta(contigs, width=70):
    out = []
    for name, seq in contigs:
        out.append('>%s some title\n' % name)
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + '\n')
    return ''.join(out).encode('ascii')


def bed_text(sites, form='plain'):
    """Lines as make_bed writes them: chrom, start, end, context, fraction, strand, depth (and --vo's probabilities)."""
    out = []
    for chrom, start, strand in sites:
        line = '%s\t%d\t%d\tNNNANNN\t0.8\t%s\t12' % (chrom, start, start + 1, strand)
        if form == 'vo':
            line += '\t0.9,0.8,0.7'
        out.append(line + '\n')
    return ''.join(out).encode('ascii')


def candidates(contigs, base):
    out = []
    for name, seq in contigs:
        s = seq.upper()
        for p, ch in enumerate(s):
            if ch == base:
                out.append((name, p, '+'))
            elif COMP.get(ch) == base:
                out.append((name, p, '-'))
    return out


def random_genome(seed, lengths, letters='ACGT'):
    rng = random.Random(seed)
    return [('ctg%d' % i, ''.join(rng.choice(letters) for _ in range(n))) for i, n in enumerate(lengths)]


def random_case(seed, lengths, base='A', motif='GATC', called=1, with_control=True):
    """A random genome with `motif` planted here and there; its occurrences are methylated (index `called` is the called letter), a
    fifth of the other candidates are listed in the control, a few in the bed."""
    rng = random.Random(seed)
    contigs = []
    for name, seq in random_genome(seed, lengths):
        s = list(seq)
        for _ in range(len(s) // 25):
            at = rng.randrange(0, max(1, len(s) - len(motif)))
            s[at:at + len(motif)] = motif
        contigs.append((name, ''.join(s[:len(seq)])))
    bed, control = [], []
    for name, seq in contigs:
        for p in range(len(seq)):
            for strand in '+-':
                a = p - called if strand == '+' else p - (len(motif) - 1 - called)
                if a < 0:
                    continue
                window = seq[a:a + len(motif)] if strand == '+' else revcomp(seq[a:a + len(motif)])
                if window == motif and rng.random() < 0.9:
                    bed.append((name, p, strand))
    listed = set(bed)
    for site in candidates(contigs, base):
        if site not in listed:
            r = rng.random()
            if r < 0.03:
                bed.append(site)
            elif r < 0.25:
                control.append(site)
    rng.shuffle(bed)
    return contigs, bed, (control if with_control else None)


def placed_case():
    """Windows that would leave a contig at either end, sites at 0 and at len - 1, a contig shorter than the shapes, an empty
    contig, N / lower case / IUPAC letters under an X and under a '.', a duplicate line, a site in both files, a site off base."""
    shapes = ['XX', 'X.X', 'XXXX', 'X..X.X']
    contigs = [('left', 'AGATCGATCAANGATCRGATCgatcAAGATCTTTTGATCA'),       # A at 0 and at len - 1
               ('tiny', 'AT'),                                            # shorter than most shapes
               ('none', ''),
               ('right', 'TGATCNNGATCYYGAtCAAAGATCGANCGAKCGATCT'),          # T at 0 and len - 1: candidates on '-'
               ('poly', 'GATC' * 12)]
    bed = [s for s in candidates(contigs, 'A') if s[0] in ('left', 'right', 'poly') and s[1] % 3 != 2]
    bed += [('tiny', 0, '+'), ('tiny', 1, '-')]
    bed += [bed[0], bed[5], bed[5]]                                       # duplicate lines
    bed += [('left', 1, '+'), ('right', 1, '-'), ('left', 11, '+')]        # off base: G on '+', C on '-', N
    control = [s for s in candidates(contigs, 'A') if s[1] % 3 == 2 and s[1] % 2 == 0]
    control += [bed[1], bed[2], ('poly', 0, '+')]                         # in both files; off base in the control
    return contigs, bed, control, shapes


def planted_case(seed=20, n=60000):
    """A random genome of n bases, every GATC's A listed with probability 0.9 (fully methylated, 90 % coverage); every other A is
    covered with probability 0.9 and then called with probability 0.02 (false calls)."""
    rng = random.Random(seed)
    contigs = random_genome(seed, [n])
    seq = contigs[0][1]
    bed, control = [], []
    for site in candidates(contigs, 'A'):
        _, p, strand = site
        in_gatc = seq[p - 1:p + 3] == 'GATC' if strand == '+' else seq[p - 2:p + 2] == 'GATC'      # GATC is its own reverse complement
        if rng.random() >= 0.9:
            continue
        if in_gatc or rng.random() < 0.02:
            bed.append(site)
        else:
            control.append(site)
    return contigs, bed, control
