"""The inputs of tests/test_phase_reads.py and tests/test_gpu_phase_reads.py, and the brute force both hold the host statement
against: .diffs rows of one sample written read by read, the builders with what each claims (tests/test_phase_cases.py holds them to
it), and the definition of phase_reads as dicts of reads and a loop over all pairs of a read's calls.  Nothing of
mcaller_amd.phase_reads is used here; fisher_log10p and bh_log10 are compare_genomes'."""
import math

import numpy as np

from mcaller_amd.compare_genomes import bh_log10, fisher_log10p

WAVE, GROUP, MAX_DEPTH = 64, 2048, 65535      # include/mcaller_hip.h: MC_PHASE_WAVE_ROWS, MC_PHASE_GROUP_ROWS, MC_PHASE_MAX_DEPTH


def row(chrom, read, pos, strand, meth, seven=False, values='0.5,9.0', context='GATCMGATCGA'):
    """One .diffs row: 8 fields with a probability, 7 (a --train row) without."""
    f = [chrom, read, str(pos), context, values, strand, 'm6A' if meth else 'A']
    return '\t'.join(f if seven else f + ['0.75' if meth else '0.25']) + '\n'


def text_of(reads, rng=None):
    """reads: [(chrom, read, strand, [(pos, methylated), ...])] -> the text, read after read with a read's rows in the order given, or
    (rng) every row of the file at a random place; every third row has 7 fields."""
    lines = [row(chrom, read, pos, strand, meth, seven=(i + k) % 3 == 0)
             for i, (chrom, read, strand, calls) in enumerate(reads) for k, (pos, meth) in enumerate(calls)]
    if rng is not None:
        lines = [lines[i] for i in rng.permutation(len(lines))]
    return ''.join(lines).encode()


def write(tmp_path, text, name='reads.diffs.1'):
    p = str(tmp_path / name)
    open(p, 'wb').write(text)
    return p


def planted_reads(rng, positions, n_reads, lo, hi, chrom='chr1', strand='+', tag='r', every=4, noise=0.05):
    """n_reads reads, each over a run of lo .. hi consecutive positions; a read belongs to one of two populations: at every
    `every`-th position population 1 is methylated and population 0 is not (with `noise`), elsewhere a coin decides."""
    reads = []
    for r in range(n_reads):
        n = int(rng.integers(lo, hi + 1))
        first = int(rng.integers(0, len(positions) - n + 1))
        pop = r & 1
        calls = []
        for i in range(first, first + n):
            meth = (pop == 1) != (rng.random() < noise) if i % every == 0 else rng.random() < 0.5
            calls.append((positions[i], bool(meth)))
        reads.append((chrom, '%s%d' % (tag, r), strand, calls))
    return reads


# ---- the cases the GPU tests expect the device to make: name -> (text, options, what it claims) ----
def case_read_lengths(lengths=(1, 2, WAVE - 1, WAVE, WAVE + 1, GROUP), seed=3):
    """One read of every length in `lengths` over sites one base apart, behind eight planted reads over the first 40 sites (the pairs
    that are written); max_dist 3: W = 3."""
    rng = np.random.default_rng([seed, len(lengths)])
    positions = list(range(1000, 1000 + max(max(lengths), 40)))
    reads = planted_reads(rng, positions[:40], 8, 40, 40, tag='p')
    for n in lengths:
        reads.append(('chr1', 'len%d' % n, '+', [(positions[i], bool(rng.random() < 0.5)) for i in range(n)]))
    return text_of(reads), dict(depth=1, max_dist=3, min_reads=4, min_margin=1), dict(lengths=lengths, window=3)


def case_shuffled(seed=11, newline=True):
    """14 reads over all of 30 sites ten bases apart, 420 lines with every row at a random place: every read spans both 256-line
    staging tiles; max_dist 50: W = 5."""
    rng = np.random.default_rng([seed, 30])
    positions = [200 + 10 * i for i in range(30)]
    text = text_of(planted_reads(rng, positions, 14, 30, 30), rng)
    return (text if newline else text[:-1]), dict(depth=10, max_dist=50, min_reads=10, min_margin=2), dict(lines=420, window=5)


def case_distance_edge(seed=17, max_dist=40):
    """Three sites: B exactly max_dist behind A, C max_dist + 1 behind B: (A, B) is a pair, (B, C) and (A, C) are none."""
    rng = np.random.default_rng([seed, max_dist])
    positions = [100, 100 + max_dist, 100 + 2 * max_dist + 1]
    return (text_of(planted_reads(rng, positions, 24, 3, 3, every=1, noise=0.2), rng), dict(depth=15, max_dist=max_dist, min_reads=10, min_margin=2),
            dict(positions=positions, window=1))


def case_window_one(seed=19):
    """Twelve sites 30 apart under max_dist 40: every site has one site behind it within reach, W = 1."""
    rng = np.random.default_rng([seed, 12])
    positions = [500 + 30 * i for i in range(12)]
    return text_of(planted_reads(rng, positions, 30, 6, 12, every=2), rng), dict(depth=10, max_dist=40, min_reads=8, min_margin=2), dict(window=1)


def case_one_wide_window(seed=23):
    """Ten sites 100 apart (w = 0 under max_dist 40) and, behind them, a cluster of twelve sites 3 apart: the cluster's first site
    alone has w = 11."""
    rng = np.random.default_rng([seed, 22])
    positions = [100 * i for i in range(1, 11)] + [5000 + 3 * i for i in range(12)]
    return text_of(planted_reads(rng, positions, 20, 22, 22, every=3), rng), dict(depth=10, max_dist=40, min_reads=8, min_margin=2), dict(window=11)


def case_strands_and_chroms(seed=29):
    """The same six positions on two chroms and two strands: four groups that must not pair across."""
    rng = np.random.default_rng([seed, 4])
    positions = [300 + 7 * i for i in range(6)]
    reads = []
    for chrom in ('chrA', 'chrB'):
        for strand in '+-':
            reads += planted_reads(rng, positions, 16, 6, 6, chrom, strand, tag='%s%s' % (chrom, 'f' if strand == '+' else 'r'), every=2)
    return text_of(reads, rng), dict(depth=12, max_dist=20, min_reads=10, min_margin=2), dict(groups=4, window=2)


def case_below_depth_between(seed=31):
    """A and C 20 apart with 18 reads each, B between them with 5: B is below -d 15 and stands in no row, (A, C) is written."""
    rng = np.random.default_rng([seed, 3])
    reads = []
    for r in range(18):
        pop = r & 1
        calls = [(700, pop == 1), (720, (pop == 1) != (r % 7 == 0))]
        if r < 5:
            calls.insert(1, (710, bool(rng.random() < 0.5)))
        reads.append(('chr1', 'b%d' % r, '-', calls))
    return text_of(reads, rng), dict(depth=15, max_dist=25, min_reads=10, min_margin=2), dict(kept=[700, 720], window=1)


def case_depth_cap(n=MAX_DEPTH, shared=24):
    """A site of n reads of one row each and, one base behind, a site the first `shared` of them also cover."""
    reads = [('chr1', 'd%d' % r, '+', [(500, r % 2 == 0)] + ([(501, r % 4 < 2)] if r < shared else [])) for r in range(n)]
    return text_of(reads), dict(depth=15, max_dist=5, min_reads=10, min_margin=2), dict(depth=n)


DEVICE_CASES = {'read_lengths': case_read_lengths, 'shuffled': case_shuffled, 'shuffled_no_newline': lambda: case_shuffled(newline=False),
                'distance_edge': case_distance_edge, 'window_one': case_window_one, 'one_wide_window': case_one_wide_window,
                'strands_and_chroms': case_strands_and_chroms, 'below_depth_between': case_below_depth_between}


def case_counter_memory(seed=37):
    """300 sites one base apart, 16 reads over all of them, max_dist 100: 30000 counters of 8 bytes beside 9 columns and the sort
    buffers -- over 2 MB, where the text (under 200 KB) and its tables are well under one."""
    rng = np.random.default_rng([seed, 300])
    return text_of(planted_reads(rng, list(range(2000, 2300)), 16, 300, 300)), dict(depth=15, max_dist=100, min_reads=10, min_margin=2), dict(window=100)


def case_many_reads(seed=41):
    """Four sites and 120 reads: a key table of 64 slots holds the sites and not the reads."""
    rng = np.random.default_rng([seed, 120])
    return text_of(planted_reads(rng, [10, 20, 30, 40], 120, 2, 4, every=2)), dict(depth=15, max_dist=30, min_reads=10, min_margin=2), dict(reads=120)


# ---- the brute force ----
def parse(path):
    """[(chrom, read, pos text, context, strand, methylated)] of the file's lines (sound files only)."""
    out = []
    for line in open(path, 'r'):
        f = line.split('\t')
        out.append((f[0], f[1], f[2], f[3], f[5], f[6][:1] == 'm'))
    return out


def brute_tables(path, depth, max_dist):
    """-> (kept sites in first-row order as (chrom, pos text, strand), {site: (context, N)}, {(A, B): [n11, n10, n01, n00]} over all
    pairs of kept sites with a shared read, calls per read key as {key: [(pos text, methylated)]}, duplicates)."""
    calls, sites, duplicates = {}, {}, 0
    for chrom, read, pos, context, strand, meth in parse(path):
        mine = calls.setdefault((chrom, read, strand), [])
        if any(p == pos for p, _ in mine):
            duplicates += 1
            continue
        mine.append((pos, meth))
        if (chrom, pos, strand) not in sites:
            sites[(chrom, pos, strand)] = [context, 0]
        sites[(chrom, pos, strand)][1] += 1
    kept = [s for s in sites if sites[s][1] >= depth]
    tables, is_kept = {}, set(kept)
    for (chrom, read, strand), mine in calls.items():
        at = [((chrom, pos, strand), int(pos), meth) for pos, meth in mine if (chrom, pos, strand) in is_kept]
        for a, int_a, meth_a in at:
            for b, int_b, meth_b in at:
                if 0 < int_b - int_a <= max_dist:
                    tables.setdefault((a, b), [0, 0, 0, 0])[(0 if meth_a else 2) + (0 if meth_b else 1)] += 1
    return kept, sites, tables, calls, duplicates


def brute_phi(n11, n10, n01, n00):
    return float(n11 * n00 - n10 * n01) / (math.sqrt(float((n11 + n10) * (n01 + n00))) * math.sqrt(float((n11 + n01) * (n10 + n00))))


def brute(path, depth=15, max_dist=1000, min_reads=10, min_margin=2, fdr=False, threshold=2.0):
    """-> (rows, reads rows, bed lines -- bytes --, figures as last_phase has them, [(table, L)] of the rows written)."""
    kept, sites, tables, calls, duplicates = brute_tables(path, depth, max_dist)
    order = {s: i for i, s in enumerate(kept)}
    pairs = [(a, b) for (a, b), (n11, n10, n01, n00) in tables.items()
             if n11 + n10 + n01 + n00 >= min_reads and min(n11 + n10, n01 + n00, n11 + n01, n10 + n00) >= min_margin]
    pairs.sort(key=lambda ab: (order[ab[0]], int(ab[1][1]), order[ab[1]]))
    rows, logs = [], []
    for a, b in pairs:
        n11, n10, n01, n00 = tables[(a, b)]
        L = fisher_log10p(n11, n11 + n10, n01, n01 + n00)
        logs.append(L)
        rows.append([a[0], a[2], a[1], b[1], str(n11 + n10 + n01 + n00), str(n11), str(n10), str(n01), str(n00),
                     str(np.round(brute_phi(n11, n10, n01, n00), 3)), str(np.round(0.0 - L, 3))])
    if fdr and rows:
        for f, q in zip(rows, bh_log10(logs)):
            f.append(str(np.round(0.0 - q, 3)))
    links = {s: 0 for s in kept}
    for (a, b), f in zip(pairs, rows):
        if float(f[-1]) >= threshold:
            links[a] += 1
            links[b] += 1
    bed = ['\t'.join((s[0], s[1], str(int(s[1]) + 1), sites[s][0], str(links[s]), s[2], str(sites[s][1]))) + '\n' for s in kept if links[s] > 0]
    read_rows = []
    for (chrom, read, strand), mine in calls.items():
        at = [(int(pos), meth) for pos, meth in mine if (chrom, pos, strand) in order]
        if at:
            read_rows.append('\t'.join((chrom, read, strand, str(min(p for p, _ in at)), str(max(p for p, _ in at)), str(len(at)),
                                        str(sum(1 for _, m in at if m)))) + '\n')
    figures = dict(n_sites=len(kept), n_pairs=len(rows), n_reads=len(read_rows), n_linked=len(bed), n_duplicates=duplicates)
    return (''.join('\t'.join(f) + '\n' for f in rows).encode(), ''.join(read_rows).encode(), ''.join(bed).encode(), figures,
            [(tables[p], L) for p, L in zip(pairs, logs)])
