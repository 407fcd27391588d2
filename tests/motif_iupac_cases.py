"""find_motifs --iupac restated by brute force -- every one of the 15^(k-1) patterns of a table as Python sets, purity tested member
by member, no code shared with mcaller_amd/find_motifs.py -- and the inputs the CPU and GPU tests share.  Feasible up to 4 or 5 X."""
import itertools
import random
import re

from tests import motif_sites as MS

SETS = {'A': 'A', 'C': 'C', 'G': 'G', 'T': 'T', 'R': 'AG', 'Y': 'CT', 'S': 'CG', 'W': 'AT', 'K': 'GT', 'M': 'AC', 'B': 'CGT', 'D': 'AGT',
        'H': 'ACT', 'V': 'ACG', 'N': 'ACGT'}
BIT = {'A': 1, 'C': 2, 'G': 4, 'T': 8}
LETTER_OF = {frozenset(v): k for k, v in SETS.items()}


def mask_of(letters):
    return sum(BIT[ch] for ch in letters)


def brute_iupac(contigs, bed, control, base='A', shapes=None, min_sites=20, min_fraction=0.5, keep_all=False):
    """-> (the text, dict(n_good, n_pure, n_maximal, n_selected))."""
    tables = MS.brute_tables(contigs, bed, control, base, shapes)
    xs_of = [[i for i in range(len(s)) if s[i] == 'X'] for s in shapes]

    def good(si, j, letters):
        t = tables.get((si, j, ''.join(letters)))
        return t is not None and t[1] >= 1 and t[2] / t[1] >= min_fraction
    n_good = sum(1 for (si, j, letters) in tables if good(si, j, letters))
    all_sets = [frozenset(v) for v in SETS.values()]
    pure = {}                                    # (si, j) -> the set of pure patterns, a pattern: a tuple of frozensets, one per X
    for si, xs in enumerate(xs_of):
        for j in range(len(xs)):
            choices = [[frozenset(base)] if i == j else all_sets for i in range(len(xs))]
            pure[si, j] = set(p for p in itertools.product(*choices) if all(good(si, j, m) for m in itertools.product(*p)))
    rows, n_maximal = [], 0
    for (si, j), patterns in pure.items():
        xs = xs_of[si]
        for p in patterns:
            grown = [p[:i] + (p[i] | {ch},) + p[i + 1:] for i in range(len(xs)) if i != j for ch in 'ACGT' if ch not in p[i]]
            if any(g in patterns for g in grown):
                continue
            n_maximal += 1
            sums = [0, 0, 0]
            for m in itertools.product(*p):
                t = tables[si, j, ''.join(m)]
                sums = [a + b for a, b in zip(sums, t)]
            if sums[2] >= min_sites and sums[2] / sums[1] >= min_fraction:
                rows.append((-sums[2], -(sums[2] / sums[1]), si, j, tuple(mask_of(s) for s in p), p, sums))
    n_selected = len(rows)
    if not keep_all:
        kept = []
        for row in rows:
            si, j, p = row[2], row[3], row[5]
            mine = {x - xs_of[si][j]: s for x, s in zip(xs_of[si], p)}
            redundant = False
            for (ui, uj), patterns in pure.items():
                theirs = [x - xs_of[ui][uj] for x in xs_of[ui]]
                if len(theirs) < len(mine) and all(r in mine for r in theirs) and tuple(mine[r] for r in theirs) in patterns:
                    redundant = True
            if not redundant:
                kept.append(row)
        rows = kept
    rows.sort(key=lambda r: r[:5])
    out = []
    for _, _, si, j, _, p, (nG, nC, nM) in rows:
        spec, it = '', iter(p)
        for ch in shapes[si]:
            spec += LETTER_OF[next(it)] if ch == 'X' else 'N'
        out.append('%s:%d\t%d\t%d\t%d\t%r\n' % (spec, xs_of[si][j] + 1, nG, nC, nM, nM / nC))
    counts = dict(n_good=n_good, n_pure=sum(len(v) for v in pure.values()), n_maximal=n_maximal, n_selected=n_selected)
    return ''.join(out).encode('ascii'), counts


def sites_matching(contigs, motif, called):
    """Every (chrom, position, strand) whose base is letter `called` (0-based) of an occurrence of the IUPAC `motif` on its strand."""
    pattern = re.compile('(?=%s)' % ''.join('[%s]' % SETS[ch] for ch in motif))
    out = []
    for name, seq in contigs:
        for hit in pattern.finditer(seq):
            out.append((name, hit.start() + called, '+'))
        rc = MS.revcomp(seq)
        for hit in pattern.finditer(rc):
            out.append((name, len(seq) - 1 - (hit.start() + called), '-'))
    return sorted(set(out))


def planted_genome(seed, n, plants):
    """A random genome of n bases with every (concrete motif, times) of `plants` written over it at random places."""
    rng = random.Random(seed)
    s = list(MS.random_genome(seed, [n])[0][1])
    for motif, times in plants:
        for _ in range(times):
            at = rng.randrange(0, n - len(motif))
            s[at:at + len(motif)] = motif
    return [('ctg0', ''.join(s))]


def gantc(seed=5, n=4000, times=25):
    """GANTC planted with every middle letter; the A of every occurrence is methylated, nothing else is."""
    contigs = planted_genome(seed, n, [('GA%sTC' % ch, times) for ch in 'ACGT'])
    return contigs, sites_matching(contigs, 'GANTC', 1)


def blocks(units):
    """A contig of the units (word, times), an N between any two: no window spans two units."""
    return [('blocks', 'N'.join(word for word, times in units for _ in range(times)))]


def noisy(seed=77, n=3000, p=0.04):
    """A random genome with a few per cent of its candidates called at random and as many covered without a call: hundreds of
    good entries at --min_sites 1 -> (contigs, bed, control)."""
    rng = random.Random(seed)
    contigs = MS.random_genome(seed, [n])
    bed, control = [], []
    for site in MS.candidates(contigs, 'A'):
        r = rng.random()
        if r < p:
            bed.append(site)
        elif r < 2 * p:
            control.append(site)
    return contigs, bed, control


def cases():
    """name -> (contigs, bed, control or None, keywords of find_motifs)."""
    out = {}
    contigs, bed = gantc()
    out['gantc'] = (contigs, bed, None, dict(shapes=['XXXXX'], min_sites=5))
    # one member just below min_fraction: GACTC keeps fewer than half of its sites
    member = sites_matching(contigs, 'GACTC', 1)
    dropped = set(member[(len(member) + 1) // 2 - 1:])
    out['member_below'] = (contigs, [s for s in bed if s not in dropped], None, dict(shapes=['XXXXX'], min_sites=5))
    # one member never covered: the GAGTC sites are in neither file, every other candidate is in one of them
    member = set(sites_matching(contigs, 'GAGTC', 1))
    listed = set(bed)
    out['member_uncovered'] = (contigs, [s for s in bed if s not in member], [s for s in MS.candidates(contigs, 'A') if s not in listed],
                               dict(shapes=['XXXXX'], min_sites=5))
    small, small_bed = gantc(6, 1500, 6)
    out['sum_reaches'] = (small, small_bed, None, dict(shapes=['XXXXX']))
    gatc = planted_genome(7, 3000, [('GATC', 60)])
    gatc_bed = sites_matching(gatc, 'GATC', 1)
    out['gatcn'] = (gatc, gatc_bed, None, dict(shapes=['XXXX', 'XXXXX'], min_sites=5))
    out['gatcn_all'] = (gatc, gatc_bed, None, dict(shapes=['XXXX', 'XXXXX'], min_sites=5, keep_all=True))
    out['two_shapes'] = (contigs, bed, None, dict(shapes=['XXXXX', 'XX.XX'], min_sites=5))
    rnd = MS.random_genome(8, [3000])
    out['shared_member'] = (rnd, sorted(set(sites_matching(rnd, 'GAY', 1) + sites_matching(rnd, 'CAC', 1))), None, dict(shapes=['XXX'], min_sites=5))
    tie = blocks([('AAC', 3), ('CAC', 2), ('GAG', 5)])
    out['ties'] = (tie, sites_matching(tie, 'NAN', 1), None, dict(shapes=['XXX'], min_sites=1))
    ccwgg = planted_genome(9, 3000, [('CCAGG', 30), ('CCTGG', 30)])
    out['base_c'] = (ccwgg, sites_matching(ccwgg, 'CCWGG', 1), None, dict(shapes=['XXX', 'XXXXX'], min_sites=5, base='C'))
    return out
