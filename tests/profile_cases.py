"""motif_profile restated by brute force -- plain loops over strings and Python floats, no code shared with
mcaller_amd/motif_profile.py -- and the cases the CPU and GPU tests share.  Every case names the edge it is there for and carries
claims about the brute force's result (tests/test_profile_cases.py holds them): a case cannot silently stop exercising its edge."""
import functools
import random

from tests import motif_sites as MS

SETS = {'A': 'A', 'C': 'C', 'G': 'G', 'T': 'T', 'R': 'AG', 'Y': 'CT', 'S': 'CG', 'W': 'AT', 'K': 'GT', 'M': 'AC',
        'B': 'CGT', 'D': 'AGT', 'H': 'ACT', 'V': 'ACG', 'N': 'ACGT'}
COMP_LETTER = {k: [k2 for k2, v2 in SETS.items() if set(v2) == set(MS.COMP[c] for c in v)][0] for k, v in SETS.items()}


def parse(entry, base):
    """'MOTIF[:I+J]' -> (letters, 0-based called offsets, canonical text)."""
    motif, _, idx = entry.upper().partition(':')
    offs = sorted(set(int(t) - 1 for t in idx.split('+'))) if idx else [i for i, ch in enumerate(motif) if ch == base]
    return motif, offs, '%s:%s' % (motif, '+'.join(str(o + 1) for o in offs))


def brute_sites(seq, motif, offs):
    """{(position, strand)}: every called letter of every occurrence, a loop per strand and start."""
    m, sites = len(motif), set()
    rc = ''.join(COMP_LETTER[ch] for ch in reversed(motif))
    for strand, letters, called in (('+', motif, offs), ('-', rc, [m - 1 - o for o in offs])):
        for start in range(len(seq) - m + 1):
            if all(seq[start + i] in 'ACGT' and seq[start + i] in SETS[letters[i]] for i in range(m)):
                for j in called:
                    sites.add((start + j, strand))
    return sites


class Result(object):
    pass


def brute(contigs, bed, control, motifs, base='A', window=0, min_sites=5, neighbours=None, min_shared=2):
    """-> Result: profile and nn (bytes), rows [(chrom, start, end, spec, nG, nC, nM)], nn_rows [(bin, bin2, shared, d)], bins
    [(chrom, start, end)], counts {(bin, motif): (nG, nC, nM)}, n_bins, n_rows, n_off_base, n_defined, n_pairs."""
    ref = {}
    for name, seq in contigs:
        ref[name] = seq.upper()
    entries = [parse(e, base) for e in motifs.split(',')]
    meth, ctl = set(bed), (None if control is None else set(control))
    R = Result()
    R.n_off_base = 0
    for name, p, strand in meth | (ctl or set()):
        on_strand = ref[name][p] if strand == '+' else MS.COMP.get(ref[name][p])
        R.n_off_base += on_strand != base
    R.bins, R.counts, R.rows = [], {}, []
    for name, seq in ref.items():
        edges = [(0, len(seq))] if window == 0 else [(a, min(a + window, len(seq))) for a in range(0, len(seq), window)]
        sites = [brute_sites(seq, motif, offs) for motif, offs, _ in entries]
        for a, b in edges:
            bi = len(R.bins)
            R.bins.append((name, a, b))
            for m, (_, _, text) in enumerate(entries):
                nG = nC = nM = 0
                for p, strand in sites[m]:
                    if a <= p < b:
                        is_meth = (name, p, strand) in meth
                        nG += 1
                        nM += is_meth
                        nC += True if ctl is None else (is_meth or (name, p, strand) in ctl)
                R.counts[bi, m] = (nG, nC, nM)
                if nG > 0:
                    R.rows.append((name, a, b, text, nG, nC, nM))
    R.profile = ''.join('%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n' % (r + ('NA' if r[5] == 0 else repr(r[6] / r[5]),)) for r in R.rows).encode('latin-1')
    B, M = len(R.bins), len(entries)
    value = [{m: R.counts[b, m][2] / R.counts[b, m][1] for m in range(M) if R.counts[b, m][1] >= min_sites} for b in range(B)]
    R.n_bins, R.n_rows, R.n_defined, R.n_pairs, R.nn_rows = B, len(R.rows), sum(1 for v in value if v), 0, []
    if neighbours is not None:
        for a in range(B):
            found = []
            for b in range(B):
                S = [m for m in range(M) if m in value[a] and m in value[b]]
                if a == b or len(S) < min_shared:
                    continue
                total = 0.0
                for m in S:
                    total = total + abs(value[a][m] - value[b][m])
                found.append((total / float(len(S)), b, len(S)))
            R.n_pairs += len(found)
            found.sort(key=lambda t: (t[0], t[1]))
            if value[a]:
                R.nn_rows += [(a, b, shared, d) for d, b, shared in found[:neighbours]]
    R.nn = ''.join('%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n' % (R.bins[a] + R.bins[b] + (shared, repr(d))) for a, b, shared, d in R.nn_rows).encode('latin-1')
    return R


class Case(object):
    """contigs: [(id, sequence as in the file)]; bed, control: [(chrom, start, strand)] (control may be None); kw: what
    motif_profile takes beside the files (motifs, base, window, min_sites, neighbours, min_shared); claims: [(what, f(Result))]."""

    def __init__(self, name, contigs, bed, control, claims, **kw):
        self.name, self.contigs, self.bed, self.control, self.claims, self.kw = name, contigs, bed, control, claims, kw


def listed(contigs, seed, p_bed=0.5, p_ctl=0.3, base='A'):
    rng = random.Random(seed)
    bed, ctl = [], []
    for site in MS.candidates(contigs, base):
        r = rng.random()
        if r < p_bed:
            bed.append(site)
        elif r < p_bed + p_ctl:
            ctl.append(site)
    rng.shuffle(bed)
    return bed, ctl


M64 = ','.join('%sA%s%s:2' % (x, y, z) for x in 'ACGT' for y in 'ACGT' for z in 'ACGT')           # 64 motifs, every xAyz
M5 = 'A:1,CA:2,GA:2,TA:2,AC:1'


def _row(R, chrom, start, spec):
    return [r for r in R.rows if r[0] == chrom and r[1] == start and r[3] == spec]


def many_contigs(seed, B, length=40):
    """B short contigs of two kinds of methylation: even ones mostly methylated, odd ones mostly not, each with noise."""
    contigs = MS.random_genome(seed, [length + (i % 7) for i in range(B)])
    rng = random.Random(seed + 1)
    bed = [s for s in MS.candidates(contigs, 'A') if rng.random() < (0.8 if int(s[0][3:]) % 2 == 0 else 0.25)]
    return contigs, bed


def build():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    m32 = 'GATC' * 8
    add('motifs_of_1_and_32_letters_straddling_a_word', [('w', 'C' * 50 + m32 + 'C' * 50)], [('w', 51, '+'), ('w', 80, '-')], None,
        [('the 32-mer occurs once a strand, over base 64', lambda R: _row(R, 'w', 0, m32 + ':2')[0][4:] == (2, 2, 2)),
         ('the 1-mer marks every A and T', lambda R: _row(R, 'w', 0, 'A:1')[0][4] == 16)],
        motifs=m32 + ':2,A:1')
    seq = 'C' * 62 + 'GATC' + 'C' * 61 + 'GATC' + 'C' * 69
    add('occurrence_over_a_window_edge_called_letter_on_either_side', [('e', seq)], [('e', 63, '+'), ('e', 129, '-')], None,
        [('A at 63 in bin 0, its T at 64 in bin 1', lambda R: _row(R, 'e', 0, 'GATC:2')[0][4:] == (1, 1, 1) and _row(R, 'e', 64, 'GATC:2')[0][4:] == (1, 1, 0)),
         ('G at 127 in bin 1, A at 128 and T at 129 in bin 2: a palindrome marks both strands at different positions',
          lambda R: _row(R, 'e', 128, 'GATC:2')[0][4:] == (2, 2, 1)),
         ('the last window is short', lambda R: R.bins[-1] == ('e', 192, 200))],
        motifs='GATC:2', window=64)
    add('called_letters_at_both_contig_ends_and_contigs_shorter_than_the_motif',
        [('ends', 'ATCCCCGA'), ('one', 'A'), ('short', 'GA'), ('none', ''), ('t', 'T')],
        [('ends', 0, '+'), ('ends', 7, '+'), ('one', 0, '+'), ('t', 0, '-')], None,
        [('AT:1 at base 0, GA:2 at the last base', lambda R: _row(R, 'ends', 0, 'AT:1')[0][4:] == (2, 2, 1) and _row(R, 'ends', 0, 'GA:2')[0][4:] == (2, 2, 1)),
         ('a contig of one base has a site of the 1-mer on either strand', lambda R: _row(R, 'one', 0, 'A:1')[0][4:] == (1, 1, 1) and _row(R, 't', 0, 'A:1')[0][4:] == (1, 1, 1)),
         ('GATC does not fit into GA', lambda R: not _row(R, 'short', 0, 'GATC:2') and _row(R, 'short', 0, 'GA:2')),
         ('the empty contig is a bin without rows', lambda R: R.n_bins == 5 and not [r for r in R.rows if r[0] == 'none'])],
        motifs='AT:1,GA:2,GATC:2,A:1')
    add('n_and_lower_case_inside_an_occurrence', [('x', 'CGANCCgatcCCGATCCGAtNC')], [('x', 7, '+')], None,
        [('the N matches nothing, lower case matches as its capital', lambda R: _row(R, 'x', 0, 'GATC:2')[0][4:] == (4, 4, 1)),
         ('GANC of the motif matches the letters, not the reference N', lambda R: _row(R, 'x', 0, 'GANC:2')[0][4] == 4)],
        motifs='GATC:2,GANC:2')
    add('overlapping_occurrences', [('o', 'AAAA'), ('p', 'CAAAAC')], [('o', 0, '+'), ('o', 3, '+')], None,
        [('AA:1+2 on AAAA: four sites', lambda R: _row(R, 'o', 0, 'AA:1+2')[0][4:] == (4, 4, 2) and _row(R, 'p', 0, 'AA:1+2')[0][4] == 4)],
        motifs='AA:1+2')
    contigs = MS.random_genome(3, [300])
    bed, ctl = listed(contigs, 4)
    add('two_motifs_sharing_sites', contigs, bed, ctl,
        [('every site of GATC:2 is one of NATC:2', lambda R: 0 < R.counts[0, 0][0] < R.counts[0, 1][0]),
         ('and of A:1', lambda R: R.counts[0, 1][0] < R.counts[0, 2][0])],
        motifs='GATC:2,NATC:2,A:1')
    contigs = MS.random_genome(5, [63, 64, 65, 128, 130])
    bed, ctl = listed(contigs, 6)
    for window, n_bins in ((64, 1 + 1 + 2 + 2 + 3), (65, 1 + 1 + 1 + 2 + 2), (100, 1 + 1 + 1 + 2 + 2)):
        add('window_%d_on_contigs_of_63_64_65_128_130' % window, contigs, bed, ctl,
            [('the bins', lambda R, n=n_bins: R.n_bins == n),
             ('a short last window', lambda R, w=window: any(a > 0 and b - a < w for _, a, b in R.bins)),
             ('all three counts differ somewhere', lambda R: any(r[4] > r[5] > r[6] > 0 for r in R.rows))],
            motifs='A:1,CA:2,GATC:2', window=window)
    add('window_65_without_control', contigs, bed, None,
        [('every site is covered', lambda R: all(r[4] == r[5] for r in R.rows))], motifs='A:1,CA:2', window=65)
    contigs = [('with', 'GATCGATCCC'), ('without', 'CCCGGGCCC'), ('uncovered', 'CCGATCCC')]
    add('a_bin_without_a_site_and_a_covered_count_of_0_and_a_site_off_base', contigs,
        [('with', 1, '+'), ('with', 0, '+'), ('without', 3, '-')], [('with', 6, '-'), ('with', 2, '+')],
        [('no row for the bin without a site', lambda R: not [r for r in R.rows if r[0] == 'without']),
         ('NA where nothing is covered', lambda R: R.profile.endswith(b'uncovered\t0\t8\tGATC:2\t2\t0\t0\tNA\n')),
         ('listed sites off base', lambda R: R.n_off_base == 3)],
        motifs='GATC:2')
    contigs = MS.random_genome(7, [70 + i for i in range(65)])
    bed, ctl = listed(contigs, 8, 0.5, 0.4)
    add('64_motifs_sparsely_defined', contigs, bed, ctl,
        [('64 motifs', lambda R: len({r[3] for r in R.rows}) == 64),
         ('the shared motifs differ pair by pair', lambda R: len({r[2] for r in R.nn_rows}) >= 4),
         ('16 lines a bin', lambda R: len(R.nn_rows) == 16 * 65)],
        motifs=M64, min_sites=1, neighbours=16, min_shared=1)
    for B, K in ((1, 3), (2, 16), (63, 1), (64, 16), (65, 5), (257, 16)):
        contigs, bed = many_contigs(100 + B, B)
        add('neighbours_of_%d_bins_k_%d' % (B, K), contigs, bed, None,
            [('every bin has min(K, B - 1) lines', lambda R, B=B, K=K: len(R.nn_rows) == B * min(K, B - 1) and R.n_pairs == B * (B - 1)),
             ('empty for one bin', lambda R, B=B: (R.nn == b'') == (B == 1))],
            motifs=M5, min_sites=2, neighbours=K, min_shared=2)
    same = MS.random_genome(9, [80])[0][1]
    contigs = [('same%d' % i, same) for i in range(20)]
    bed = [(name, p, s) for name, _ in contigs for _, p, s in MS.candidates([('x', same)], 'A') if p % 3]
    add('identical_profiles_the_index_decides', contigs, bed, None,
        [('every distance is 0.0', lambda R: all(r[3] == 0.0 for r in R.nn_rows)),
         ('the four smallest other indices', lambda R: [r[1] for r in R.nn_rows[:4]] == [1, 2, 3, 4] and [r[1] for r in R.nn_rows[8:12]] == [0, 1, 3, 4])],
        motifs=M5, min_sites=1, neighbours=4, min_shared=1)
    contigs = MS.random_genome(11, [30 + 3 * i for i in range(30)]) + [('bare', 'CCGGCCGG')]
    bed, ctl = listed(contigs, 12, 0.5, 0.3)
    add('min_shared_cuts_some_pairs', contigs, bed, ctl,
        [('some pairs have a distance, some have none', lambda R: 0 < R.n_pairs < 30 * 29),
         ('a bin with fewer than K lines', lambda R: 0 < len(R.nn_rows) < 6 * R.n_defined),
         ('a bin with no defined motif is nobody\'s neighbour', lambda R: R.n_defined < R.n_bins and all(30 not in r[:2] for r in R.nn_rows)),
         ('nCovered exactly at and one below min_sites', lambda R: {3, 4} <= {v[1] for v in R.counts.values()})],
        motifs=M5, min_sites=4, neighbours=6, min_shared=4)
    add('min_shared_cuts_all_pairs', contigs, bed, ctl,
        [('no pair has a distance', lambda R: R.n_pairs == 0 and R.nn == b'' and R.n_defined > 0)],
        motifs=M5, min_sites=4, neighbours=6, min_shared=6)
    contigs = MS.random_genome(13, [200, 131])
    bed, ctl = listed(contigs, 14, 0.5, 0.3, 'C')
    add('windows_as_neighbours_base_c', contigs, bed, ctl,
        [('windows of both contigs', lambda R: R.n_bins == 4 + 3 and len(R.nn_rows) > 0),
         ('IUPAC letters', lambda R: _row(R, 'ctg0', 0, 'CCWGG:2') is not None)],
        motifs='C:1,CCWGG:2,GC:2,RCY:2', base='C', window=64, min_sites=1, neighbours=3, min_shared=1)
    return cases


CASES = build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The brute force's Result of a case, made once and shared (nobody changes it)."""
    c = BY_NAME[name]
    return brute(c.contigs, c.bed, c.control, **c.kw)


def write(tmp_path, case):
    """The case as files -> (reference, bed, control or None)."""
    ref, pb, pc = str(tmp_path / 'ref.fasta'), str(tmp_path / 'sites.bed'), None
    open(ref, 'wb').write(MS.fasta(case.contigs))
    open(pb, 'wb').write(MS.bed_text(case.bed))
    if case.control is not None:
        pc = str(tmp_path / 'control.bed')
        open(pc, 'wb').write(MS.bed_text(case.control))
    return ref, pb, pc
