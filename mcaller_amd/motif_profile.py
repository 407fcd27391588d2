"""Per-contig motif methylation and nearest contigs: which contigs (or windows of one) carry which methyltransferase's signature?

    python -m mcaller_amd.motif_profile -r ref.fasta --bed SUMMARY.bed [--control CONTROL.bed]
                                        (--motifs SPEC[,SPEC...] | --from_report FIND_MOTIFS_OUT) [-b A] [--window 0] [--min_sites 5]
                                        [--neighbours K --nn OUT.nn [--min_shared 2]] [-o OUT] [--device]

The reference has no such program.  find_motifs answers for the genome as a whole; this module counts the same three numbers per
BIN (a contig, or a window of one) and motif, and finds every bin's nearest bins by the fractions -- the table contigs of a
metagenome are binned by and plasmids are assigned to hosts by.

Inputs.  -r, --bed and --control are read exactly as find_motifs reads them (find_motifs.read_reference, read_sites: upper-cased
contigs, of several records with one id the last; fields 1, 2 and 6 of every line; the same ValueErrors -- fewer than 6
tab-separated fields, a start int() does not take, a strand other than + / -, an unknown chrom, a start outside its contig).  A
site listed twice counts once.  A listed site whose reference base on its strand is not --base is ignored and counted (n_off_base).

Motifs.  --motifs takes 1 to 64 entries `MOTIF[:I+J+...]` in the syntax of mCaller's --motifs (refmark.parse_motifs, entry by
entry: 1 to 32 IUPAC letters, the called letters are the 1-based indices given or, without indices, every letter equal to --base;
each called letter is --base itself).  Anything parse_motifs refuses in an entry is its ValueError; no entry, more than 64 entries
and an entry given twice (by its canonical text `MOTIF:I+J`) are ValueErrors.  --from_report takes field 1 of every line of a
find_motifs output, in file order, as the entries.  Exactly one of --motifs and --from_report is given: ValueError otherwise.  A
--base other than A, C, G, T is a ValueError.

Sites.  Matching is the rule of csrc/mc_iupac.h: a sequence letter matches a motif letter iff it is one of A, C, G, T and lies in
the letter's set (an N of the reference matches nothing; the reference is upper-cased first, so a lower-case letter matches as its
capital).  Every occurrence inside a contig counts, overlapping ones included.  On '+' the motif is looked for as it stands; on '-'
its IUPAC reverse complement is looked for on the forward sequence, the called offsets mirrored.  A SITE of motif m is a (position,
strand) that is a called letter of at least one occurrence of m on that strand: a position marked by two occurrences of one motif
is one site, a site of two motifs counts under both.  A site is METHYLATED if --bed lists it and COVERED if --bed or --control
lists it; without --control every site is covered.

Bins.  --window 0: a bin is a contig, in the reference's order, its start 0 and its end the contig's length.  --window W, an
integer W >= 64: the bins of a contig of length L are [iW, min((i + 1)W, L)) for i = 0, 1, ..., contig after contig (a contig of
no bases has none).  A site belongs to the bin of its own position, whatever bin the rest of the occurrence lies in.  Any other
--window is a ValueError.

The profile file (-o).  nGenome, nCovered, nMethylated per (bin, motif): the sites, the covered and the methylated ones.  One line
per (bin, motif) with nGenome > 0, bins in order and within a bin the motifs in the order given, tab-separated:
    chrom  start  end  SPEC  nGenome  nCovered  nMethylated  fraction
SPEC is the entry's canonical text, fraction repr(float64(nMethylated) / float64(nCovered)), or the two letters NA when nCovered
is 0.

The neighbours file (--neighbours K --nn OUT.nn; K is 1 to 16, anything else -- 17 included -- a ValueError; either option
without the other is a ValueError).  --min_sites (>= 1, default 5) and --min_shared (>= 1, default 2): smaller values are
ValueErrors.  Motif m is DEFINED in bin b when its nCovered there is >= --min_sites; its value f[b, m] is the fraction above.  For
two different bins a and b let S be the motifs defined in both, in ascending motif order.  If |S| < --min_shared the pair has no
distance; otherwise
    d(a, b) = (sum over m in S of |f[a, m] - f[b, m]|) / float64(|S|)
in IEEE fp64: per motif one subtraction, one absolute value and one addition to a sum that starts at 0.0, in S's order; then the
one division.  Every bin with at least one defined motif, in order, gets up to K lines: the bins at the smallest distance, of equal
distances the smaller bin index first; a bin with fewer than K bins at a distance gets fewer lines (none is possible).  A line is
    chrom  start  end  chrom2  start2  end2  shared  d
tab-separated, shared = |S|, d as repr(float).

`last_counts` holds n_bins, n_rows (lines of the profile file), n_off_base, n_defined (bins with at least one defined motif;
counted whether or not neighbours are asked for) and n_pairs (ordered pairs (a, b) that have a distance; 0 without --neighbours).

Out of scope: circular contigs.

`motif_profile` is that definition in NumPy (the host statement; no GPU): the sites of all contigs at once on a concatenation
that keeps 32 non-letters between contigs, the distances block by block with a loop over the motifs (the order of the additions
is the definition's; a motif outside S adds 0.0, which leaves a non-negative sum as it is).  `motif_profile_device` (--device) has
the GPU make the same bytes (Device.motif_profile: csrc/motifs/mc_motifprofile.inc) and runs the host statement whenever the device
declines; `last_report` says who made the output."""
import os
import sys

import numpy as np

from . import refmark
from .find_motifs import _CODE, _write, read_reference, read_sites

last_report = None         # what the last call did: dict(by='device' | 'host', reason=None | str, n_rows=int, n_nn_rows=int)
last_counts = None         # the host statement's figures: dict(n_bins, n_rows, n_off_base, n_defined, n_pairs)

MAX_MOTIFS = 64
MAX_NEIGHBOURS = 16
PAD = 32                   # non-letters between two contigs of the host statement's concatenation: no motif is longer
_MEMBER = {ch: np.array([c in members for c in 'ACGT'] + [False]) for ch, members in refmark.IUPAC_SETS.items()}


def parse_profile_motifs(text, base):
    """`SPEC[,SPEC...]` (or a list of entries) -> [refmark.IupacMotifs of one entry each]; ValueError for anything else."""
    entries = text.split(',') if isinstance(text, str) else list(text)
    if not 1 <= len(entries) <= MAX_MOTIFS:
        raise ValueError('--motifs: 1 to %d entries, %d given' % (MAX_MOTIFS, len(entries)))
    specs = []
    for entry in entries:
        if not isinstance(entry, str) or ',' in entry:
            raise ValueError('--motifs entry %r: one motif an entry' % (entry,))
        specs.append(refmark.parse_motifs(entry, base))
    texts = [s.text for s in specs]
    for i, t in enumerate(texts):
        if t in texts[:i]:
            raise ValueError('--motifs entry %r is given twice' % t)
    return specs


def read_report(path):
    """Field 1 of every line of a find_motifs output, in file order."""
    with open(path, 'rb') as fh:
        lines = fh.read().decode('latin-1').split('\n')
    return [line.split('\t')[0] for line in lines if line]


def _checked(base, motifs, from_report, window, min_sites, neighbours, nn, min_shared):
    base = str(base).upper()
    if base not in ('A', 'C', 'G', 'T'):
        raise ValueError('--base %r: the called base is one of A, C, G, T' % base)
    if (motifs is None) == (from_report is None):
        raise ValueError('one of --motifs and --from_report is needed, and only one')
    specs = parse_profile_motifs(read_report(from_report) if motifs is None else motifs, base)
    for name, v in (('--window', window), ('--min_sites', min_sites), ('--min_shared', min_shared)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('%s %r: an integer' % (name, v))
    if window != 0 and window < 64:
        raise ValueError('--window %d: 0 (a bin is a contig) or at least 64' % window)
    if min_sites < 1 or min_shared < 1:
        raise ValueError('--min_sites and --min_shared are at least 1')
    if (neighbours is None) != (nn is None):
        raise ValueError('--neighbours and --nn go together')
    if neighbours is not None and (isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer))
                                   or not 1 <= neighbours <= MAX_NEIGHBOURS):
        raise ValueError('--neighbours %r: 1 to %d' % (neighbours, MAX_NEIGHBOURS))
    return base, specs, int(window), int(min_sites), (None if neighbours is None else int(neighbours)), int(min_shared)


def _marks(code, letters, offsets):
    """bool [len(code)]: the called letters of every occurrence of the motif in the letter codes."""
    marks = np.zeros(len(code), dtype=bool)
    n_win = len(code) - len(letters) + 1
    if n_win <= 0:
        return marks
    starts = np.ones(n_win, dtype=bool)
    for i, ch in enumerate(letters):
        starts &= _MEMBER[ch][code[i:i + n_win]]
    for j in offsets:
        marks[j:j + n_win] |= starts
    return marks


def bins_of(lens, window):
    """-> (contig of every bin, its start, its end, the first bin of every contig [n + 1]) as int64 arrays."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    per = np.ones(len(lens), dtype=np.int64) if window == 0 else (lens + window - 1) // window
    first = np.zeros(len(lens) + 1, dtype=np.int64)
    first[1:] = np.cumsum(per)
    contig = np.repeat(np.arange(len(lens), dtype=np.int64), per)
    if window == 0:
        return contig, np.zeros(len(lens), dtype=np.int64), lens.copy(), first
    start = (np.arange(len(contig), dtype=np.int64) - first[contig]) * window
    return contig, start, np.minimum(start + window, lens[contig]), first


def count_profile(ref, specs, base, meth, control, window):
    """-> (counts int64 [bins, motifs, 3]: nGenome, nCovered, nMethylated; (contig, start, end) of the bins; n_off_base)."""
    names = list(ref)
    lens = np.array([len(ref[n]) for n in names], dtype=np.int64).reshape(-1)
    bin_contig, bin_start, bin_end, first = bins_of(lens, window)
    at = np.zeros(len(names) + 1, dtype=np.int64)                 # where the contigs stand in the concatenation
    at[1:] = np.cumsum(lens + PAD)
    G = int(at[-1])
    code = np.full(G, 4, dtype=np.uint8)
    listed = [[np.zeros(G, dtype=bool), np.zeros(G, dtype=bool)] for _ in range(2)]          # [bed, control][strand]
    for i, name in enumerate(names):
        a, b = int(at[i]), int(at[i] + lens[i])
        code[a:b] = _CODE[np.frombuffer(ref[name].encode('latin-1', 'replace'), dtype=np.uint8)]
        for s in range(2):
            listed[0][s][a:b] = meth[name][s]
            if control is not None:
                listed[1][s][a:b] = control[name][s]
    of_pos = np.repeat(np.arange(len(names), dtype=np.int64), lens + PAD)
    off = np.arange(G, dtype=np.int64) - at[of_pos]
    bin_of = of_pos if window == 0 else first[of_pos] + off // window      # (padding is never a site: its bin is never read)
    b = 'ACGT'.index(base)
    n_off_base = 0
    for s, letter in ((0, b), (1, 3 - b)):
        n_off_base += int(((listed[0][s] | listed[1][s]) & (code != letter)).sum())
    counts = np.zeros((len(bin_contig), len(specs), 3), dtype=np.int64)
    B = len(bin_contig)
    for m, spec in enumerate(specs):
        for s, table in enumerate(spec.strands()):
            letters, offsets = table[0]
            sites = _marks(code, letters, offsets)
            covered = sites if control is None else sites & (listed[0][s] | listed[1][s])
            for k, which in enumerate((sites, covered, sites & listed[0][s])):
                counts[:, m, k] += np.bincount(bin_of[which], minlength=B)[:B]
    return counts, (bin_contig, bin_start, bin_end), n_off_base


def profile_rows(names, specs, counts, bins):
    """The profile file's bytes and the number of its lines."""
    bin_contig, bin_start, bin_end = bins
    out = []
    for bi, m in np.argwhere(counts[:, :, 0] > 0).tolist():
        nG, nC, nM = counts[bi, m].tolist()
        frac = 'NA' if nC == 0 else repr(float(np.float64(nM) / np.float64(nC)))
        out.append('%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n' % (names[bin_contig[bi]], bin_start[bi], bin_end[bi], specs[m].text, nG, nC, nM, frac))
    return ''.join(out).encode('latin-1', 'replace'), len(out)


def fractions(counts, min_sites):
    """-> (f float64 [bins, motifs], 0.0 where the motif is not defined; defined bool [bins, motifs])."""
    nC, nM = counts[:, :, 1], counts[:, :, 2]
    defined = nC >= min_sites
    f = np.zeros(nC.shape, dtype=np.float64)
    f[defined] = nM[defined].astype(np.float64) / nC[defined].astype(np.float64)
    return f, defined


def neighbour_rows(names, f, defined, bins, K, min_shared, block=128):
    """The neighbours file's bytes, the number of its lines and n_pairs."""
    bin_contig, bin_start, bin_end = bins
    B, M = f.shape
    used = [m for m in range(M) if defined[:, m].any()]
    has = defined.any(axis=1)
    label = ['%s\t%d\t%d' % (names[bin_contig[i]], bin_start[i], bin_end[i]) for i in range(B)]
    out, n_pairs = [], 0
    for q0 in range(0, B, block):
        q1 = min(B, q0 + block)
        total = np.zeros((q1 - q0, B), dtype=np.float64)
        shared = np.zeros((q1 - q0, B), dtype=np.int64)
        for m in used:                                            # ascending: the order of the additions is the definition's
            both = defined[q0:q1, m, None] & defined[None, :, m]
            total += np.where(both, np.abs(f[q0:q1, m, None] - f[None, :, m]), 0.0)
            shared += both
        valid = shared >= min_shared
        valid[np.arange(q1 - q0), np.arange(q0, q1)] = False
        n_pairs += int(valid.sum())
        with np.errstate(all='ignore'):
            d = total / shared.astype(np.float64)
        order = np.argsort(np.where(valid, d, np.inf), axis=1, kind='stable')[:, :K]      # stable: of equal distances the smaller index
        for r in np.nonzero(has[q0:q1])[0].tolist():
            for c in order[r].tolist():
                if not valid[r, c]:
                    break
                out.append('%s\t%s\t%d\t%s\n' % (label[q0 + r], label[c], shared[r, c], repr(float(d[r, c]))))
    return ''.join(out).encode('latin-1', 'replace'), len(out), n_pairs


def _host(reference, bed, control, base, specs, window, min_sites, neighbours, nn, min_shared, out, reason):
    global last_report, last_counts
    last_report = last_counts = None
    ref = read_reference(reference)
    meth = read_sites(bed, ref)
    ctl = None if control is None else read_sites(control, ref)
    counts, bins, n_off_base = count_profile(ref, specs, base, meth, ctl, window)
    names = list(ref)
    data, n_rows = profile_rows(names, specs, counts, bins)
    f, defined = fractions(counts, min_sites)
    nn_data, n_nn_rows, n_pairs = (b'', 0, 0) if neighbours is None else neighbour_rows(names, f, defined, bins, neighbours, min_shared)
    if nn is not None:
        _write(nn, nn_data)
    _write(out, data)
    last_counts = dict(n_bins=len(bins[0]), n_rows=n_rows, n_off_base=n_off_base, n_defined=int(defined.any(axis=1).sum()), n_pairs=n_pairs)
    last_report = dict(by='host', reason=reason, n_rows=n_rows, n_nn_rows=n_nn_rows)
    return n_rows


def motif_profile(reference, bed, control=None, base='A', motifs=None, from_report=None, window=0, min_sites=5, neighbours=None, nn=None,
                  min_shared=2, out=None):
    """The host statement: the definition above in NumPy -> the number of lines of the profile file."""
    base, specs, window, min_sites, neighbours, min_shared = _checked(base, motifs, from_report, window, min_sites, neighbours, nn, min_shared)
    return _host(reference, bed, control, base, specs, window, min_sites, neighbours, nn, min_shared, out, 'the host statement was asked for')


def motif_profile_device(reference, bed, control=None, base='A', motifs=None, from_report=None, window=0, min_sites=5, neighbours=None,
                         nn=None, min_shared=2, out=None):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_report, last_counts
    base, specs, window, min_sites, neighbours, min_shared = _checked(base, motifs, from_report, window, min_sites, neighbours, nn, min_shared)
    last_report = last_counts = None
    from .device import get_device
    ref = read_reference(reference)
    blob, n_rows, nn_blob, n_nn_rows, reason = get_device().motif_profile(ref, path=bed, control_path=control, base=base, specs=specs,
                                                                          window=window, min_sites=min_sites, neighbours=neighbours,
                                                                          min_shared=min_shared)
    if blob is not None:
        if nn is not None:
            _write(nn, nn_blob)
        _write(out, blob)
        last_report = dict(by='device', reason=None, n_rows=n_rows, n_nn_rows=n_nn_rows)
        return n_rows
    return _host(reference, bed, control, base, specs, window, min_sites, neighbours, nn, min_shared, out, reason)


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Count the methylated sites of given motifs per contig or window, and find every contig\'s nearest contigs')
    parser.add_argument('-r', '--reference', type=str, required=True, help='fasta file with the reference the sites were called on')
    parser.add_argument('--bed', type=str, required=True, help='summary bed file from make_bed (plain, --vo or -p): the methylated sites')
    parser.add_argument('--control', type=str, required=False, help='summary from make_bed --control: covered sites that were not called')
    parser.add_argument('--motifs', type=str, required=False, help='1 to 64 motifs MOTIF[:I+J], comma-separated, in the syntax of mCaller --motifs')
    parser.add_argument('--from_report', type=str, required=False, help='take the motifs from field 1 of this find_motifs output')
    parser.add_argument('-b', '--base', type=str, required=False, default='A', help='the called base (default: A)')
    parser.add_argument('--window', type=int, required=False, default=0, help='bins of this many bases, at least 64 (default 0: a bin is a contig)')
    parser.add_argument('--min_sites', type=int, required=False, default=5, help='covered sites a motif needs in a bin to be defined there (default: 5)')
    parser.add_argument('--neighbours', type=int, required=False, help='with --nn: the nearest bins of every bin, 1 to 16')
    parser.add_argument('--nn', type=str, required=False, help='with --neighbours: write the neighbours to this file')
    parser.add_argument('--min_shared', type=int, required=False, default=2, help='motifs two bins must both define to have a distance (default: 2)')
    parser.add_argument('-o', '--output', type=str, required=False, help='write the profile to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', required=False, help='count on the GPU (the host statement runs when it declines)')
    args = parser.parse_args(argv)
    if (args.motifs is None) == (args.from_report is None):
        parser.error('one of --motifs and --from_report is needed, and only one')
    if (args.neighbours is None) != (args.nn is None):
        parser.error('--neighbours and --nn go together')

    assert os.path.isfile(args.reference), 'file not found at ' + args.reference
    assert os.path.isfile(args.bed), 'file not found at ' + args.bed
    assert args.control is None or os.path.isfile(args.control), 'file not found at ' + args.control
    assert args.from_report is None or os.path.isfile(args.from_report), 'file not found at ' + args.from_report

    run = motif_profile_device if args.device else motif_profile
    n = run(args.reference, args.bed, args.control, args.base, args.motifs, args.from_report, args.window, args.min_sites, args.neighbours,
            args.nn, args.min_shared, args.output)
    if args.device and last_report['by'] == 'host':
        sys.stderr.write('motif_profile: %s; the host statement made the output\n' % last_report['reason'])
    return n


if __name__ == '__main__':
    main()
