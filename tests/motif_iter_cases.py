"""find_motifs --iterative restated by brute force -- a Python loop per candidate, letter by letter, no code shared with
mcaller_amd/find_motifs.py -- and the inputs the CPU and GPU tests share."""
import itertools
import random

from tests import motif_iupac_cases as IC
from tests import motif_sites as MS


def windows(contigs, base, shapes):
    """Every (site, shape index, j, the letters under the X) whose window counts, by a loop over every candidate, shape and X."""
    for name, seq in [(n, s.upper()) for n, s in dict(contigs).items()]:
        for p in range(len(seq)):
            for strand in '+-':
                if (seq[p] if strand == '+' else MS.COMP.get(seq[p])) != base:
                    continue
                for si, shape in enumerate(shapes):
                    W = len(shape)
                    xs = [i for i in range(W) if shape[i] == 'X']
                    for j, o in enumerate(xs):
                        a, b = (p - o, p - o + W) if strand == '+' else (p - (W - 1 - o), p + o + 1)
                        if a < 0 or b > len(seq):
                            continue
                        window = seq[a:b] if strand == '+' else MS.revcomp(seq[a:b])
                        letters = ''.join(window[x] for x in xs)
                        if all(ch in 'ACGT' for ch in letters):
                            yield (name, p, strand), si, j, letters


def tables_without(found, bed, control, explained):
    """MS.brute_tables' dictionary from `found` (list(windows(...))), the explained sites skipped."""
    meth, ctl = set(bed), (None if control is None else set(control))
    tables = {}
    for site, si, j, letters in found:
        if site in explained:
            continue
        t = tables.setdefault((si, j, letters), [0, 0, 0])
        t[0] += 1
        t[1] += True if ctl is None else (site in meth or site in ctl)
        t[2] += site in meth
    return tables


def first_iupac(tables, base, shapes, min_sites, min_fraction, keep_all):
    """The first row of the --iupac report over `tables` -> (its line, shape index, j, the sets of the X) or None.  A restatement of
    IC.brute_iupac (which counts its own tables) with one economy: a pure pattern's members are all good, so at every X only the
    letters that stand there in some good entry of the table are tried."""
    xs_of = [[i for i in range(len(s)) if s[i] == 'X'] for s in shapes]
    good = set(key for key, t in tables.items() if t[1] >= 1 and t[2] / t[1] >= min_fraction)
    pure = {}
    for si, xs in enumerate(xs_of):
        for j in range(len(xs)):
            mine = [letters for (ti, tj, letters) in good if (ti, tj) == (si, j)]
            choices = []
            for i in range(len(xs)):
                seen = sorted(set(m[i] for m in mine))
                choices.append([frozenset(c) for n in range(1, len(seen) + 1) for c in itertools.combinations(seen, n)])
            pure[si, j] = set(p for p in itertools.product(*choices) if all((si, j, ''.join(m)) in good for m in itertools.product(*p)))
    rows = []
    for (si, j), patterns in pure.items():
        for p in patterns:
            grown = [p[:i] + (p[i] | {ch},) + p[i + 1:] for i in range(len(p)) if i != j for ch in 'ACGT' if ch not in p[i]]
            if any(g in patterns for g in grown):
                continue
            sums = [sum(tables[si, j, ''.join(m)][c] for m in itertools.product(*p)) for c in range(3)]
            if sums[2] >= min_sites and sums[2] / sums[1] >= min_fraction:
                rows.append((-sums[2], -(sums[2] / sums[1]), si, j, tuple(IC.mask_of(s) for s in p), p, sums))
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
    if not rows:
        return None
    _, _, si, j, _, p, (nG, nC, nM) = min(rows, key=lambda r: r[:5])
    spec, it = '', iter(p)
    for ch in shapes[si]:
        spec += IC.LETTER_OF[next(it)] if ch == 'X' else 'N'
    return '%s:%d\t%d\t%d\t%d\t%r\n' % (spec, xs_of[si][j] + 1, nG, nC, nM, nM / nC), si, j, p


def first_plain(contigs, tables, base, shapes, min_sites, min_fraction, keep_all):
    text = MS.brute(contigs, None, None, base, shapes, min_sites, min_fraction, keep_all, tables=tables).decode('ascii')
    if not text:
        return None
    line = text[:text.index('\n') + 1]
    spec, called = line.split('\t')[0].split(':')
    # without --iupac the letters under the X are of ACGT: an N stands under a '.', and SPEC names its shape
    shape = ''.join('.' if ch == 'N' else 'X' for ch in spec)
    si = shapes.index(shape)
    xs = [i for i in range(len(shape)) if shape[i] == 'X']
    return line, si, xs.index(int(called) - 1), tuple(frozenset(spec[x]) for x in xs)


def brute_iterative(contigs, bed, control, base='A', shapes=None, min_sites=20, min_fraction=0.5, keep_all=False, iupac=False, max_motifs=16):
    """-> (the rows' text, [explained candidates per row], the --unexplained text)."""
    found = list(windows(contigs, base, shapes))
    explained, lines, n_explained = set(), [], []
    while len(lines) < max_motifs:
        tables = tables_without(found, bed, control, explained)
        if iupac:
            first = first_iupac(tables, base, shapes, min_sites, min_fraction, keep_all)
        else:
            first = first_plain(contigs, tables, base, shapes, min_sites, min_fraction, keep_all)
        if first is None:
            break
        line, si, j, sets = first
        lines.append(line)
        now = set()
        for site, ti, tj, letters in found:                # the explain step: per candidate, letter by letter
            if (ti, tj) == (si, j) and site not in explained and all(ch in s for ch, s in zip(letters, sets)):
                now.add(site)
        n_explained.append(len(now))
        explained |= now
    order = {name: i for i, name in enumerate(dict(contigs))}
    seqs = {name: seq.upper() for name, seq in dict(contigs).items()}
    left = sorted(set(s for s in bed if s not in explained and (seqs[s[0]][s[1]] if s[2] == '+' else MS.COMP.get(seqs[s[0]][s[1]])) == base),
                  key=lambda s: (order[s[0]], s[1]))
    return ''.join(lines).encode('ascii'), n_explained, ''.join('%s\t%d\t%d\t.\t.\t%s\n' % (c, p, p + 1, s) for c, p, s in left).encode('ascii')


def three_motifs(seed=31, n=6000):
    """GATC, GANTC and CCAAT planted over n bases; the A of every occurrence (the second A of CCAAT) is methylated, a few other
    candidates are false calls, most of the rest is covered -> (contigs, bed, control, keywords)."""
    rng = random.Random(seed)
    contigs = IC.planted_genome(seed, n, [('GATC', 25)] + [('GA%sTC' % ch, 5) for ch in 'ACGT'] + [('CCAAT', 25)])
    real = set(IC.sites_matching(contigs, 'GATC', 1) + IC.sites_matching(contigs, 'GANTC', 1) + IC.sites_matching(contigs, 'CCAAT', 3))
    bed, control = sorted(real), []
    for site in MS.candidates(contigs, 'A'):
        if site not in real:
            r = rng.random()
            if r < 0.01:
                bed.append(site)
            elif r < 0.9:
                control.append(site)
    return contigs, bed, control, dict(shapes=['XXXX', 'XXXXX', 'XX..XX'], min_sites=5)


def cases():
    """name -> (contigs, bed, control or None, keywords of find_motifs without iupac / iterative)."""
    out = dict(IC.cases())
    for seed, with_control in ((1, True), (2, False)):
        contigs, bed, control = MS.random_case(seed, [700, 90, 300], with_control=with_control)
        out['random%d' % seed] = (contigs, bed, control, dict(shapes=['XXX', 'XXXX', 'X.XX'], min_sites=3))
    contigs, bed, control, kw = three_motifs()
    out['three_motifs'] = (contigs, bed, control, kw)
    return out
