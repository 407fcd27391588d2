"""Compare two `make_bed --vo` BED files site by site: do the two samples' per-read methylation probabilities differ?

    python -m mcaller_amd.compare_genomes --bed1 A.bed --bed2 B.bed [-g XMFA] [-o OUT] [--device] [-v]

The reference's program of this name (compare_genomes.py) reads the two files into dictionaries keyed by (chrom, start, end,
strand) and runs four SciPy tests per shared key.  UNLIKE THE REFERENCE, sample 1 is tested against sample 2 here:
compare_genomes.py:21-29 passes bed1's probabilities as both arguments of every test, so ks_2samp(x, x) has p = 1, the
`pval4 < 0.9` filter lets nothing through and the program prints nothing for any input.  There is no p-value filter here either:
every shared key gets a row.

One row per key of bed1 that bed2 also has, in bed1's file order, tab-separated:

    chrom start end strand frac1 depth1 frac2 depth2 U z_mwu z_rs t D nlp_mwu nlp_rs nlp_t nlp_ks

frac and depth are fields 5 and 7 of the two lines as they stand; x and y are the probability lists (field 8) of the key's
line in bed1 and bed2.  U, z_mwu, nlp_mwu: mannwhitneyu(x, y, alternative='two-sided', method='asymptotic') (U of x; z is
SciPy's standardized statistic with tie and continuity correction); z_rs, nlp_rs: ranksums(x, y); t, nlp_t: ttest_ind(x, y);
D: ks_2samp's statistic, nlp_ks from Smirnov's limit kstwobign.sf(sqrt(n1 n2 / (n1 + n2)) D).  U is str(float(U)), D its repr,
z and t are str(np.round(v, 3)), every nlp is str(np.round(0.0 - np.log10(p), 3)).

`compare_by_position` is that definition written with the SciPy calls (the host statement).  `compare_by_position_device`
(--device) has the GPU make the same bytes (Device.bed_compare: csrc/compare/mc_bedcompare.hip) and runs the host statement
whenever the device declines; `last_compare` says who made the output.  -g is accepted and unused, as in the reference."""
import os
import sys
import warnings

import numpy as np

last_compare = None        # what the last comparison did: dict(by='device' | 'host', reason=None | str, n_sites=int)


def read_bed(bed):
    """{(chrom, start, end, strand): ((frac, depth), probabilities)} of a --vo BED file, the reference's loop (compare_genomes.py:
    11-16): a line that does not have 8 fields is its tuple-unpacking ValueError; a later duplicate of a key keeps the first
    position and takes the last value."""
    sites = {}
    with open(bed, 'r') as fi:
        for line in fi:
            csome, start, end, motif, perc_meth, strand, num_reads, probabilities = tuple(line.split('\t'))
            sites[(csome, start, end, strand)] = ((perc_meth, num_reads), np.asarray([float(p) for p in probabilities.strip().split(',')]))
    return sites


def site_values(x, y):
    """The nine printed values of a site, as text, from the SciPy calls of the definition."""
    from scipy.stats import ks_2samp, kstwobign, mannwhitneyu, ranksums, ttest_ind
    n1, n2 = len(x), len(y)
    n = n1 + n2
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        mwu = mannwhitneyu(x, y, alternative='two-sided', method='asymptotic')
        U1 = mwu.statistic
        # SciPy's standardized statistic (_get_mwu_z), which mannwhitneyu does not hand out
        _, counts = np.unique(np.concatenate([x, y]), return_counts=True)
        counts = counts.astype(np.float64)
        tie_term = (counts**3 - counts).sum()
        s = np.sqrt(n1 * n2 / 12 * ((n + 1) - tie_term / (n * (n - 1))))
        numerator = np.maximum(U1, n1 * n2 - U1) - n1 * n2 / 2
        numerator -= 0.5
        z_mwu = np.float64(numerator) / s
        rs = ranksums(x, y)
        tt = ttest_ind(x, y)
        D = ks_2samp(x, y, method='asymp').statistic
        p_ks = kstwobign.sf(np.sqrt(n1 * n2 / (n1 + n2)) * D)
        nlp = [str(np.round(0.0 - np.log10(p), 3)) for p in (mwu.pvalue, rs.pvalue, tt.pvalue, p_ks)]
        return [str(float(U1)), str(np.round(z_mwu, 3)), str(np.round(rs.statistic, 3)), str(np.round(tt.statistic, 3)),
                repr(float(D))] + nlp


def _write(out, data):
    """data (bytes) to `out`: None is stdout, a str a path, anything else a file object."""
    if isinstance(out, (str, os.PathLike)):
        with open(out, 'wb') as fo:
            fo.write(data)
        return
    fo = sys.stdout if out is None else out
    if hasattr(fo, 'buffer'):
        fo.flush()
        fo.buffer.write(data)
        fo.buffer.flush()
    else:
        try:
            fo.write(data.decode('ascii'))
        except TypeError:
            fo.write(data)


def compare_rows(bed1, bed2):
    """The rows of the definition as bytes, and their number."""
    sites1, sites2 = read_bed(bed1), read_bed(bed2)
    rows = []
    for pos in sites1:
        if pos in sites2:
            (frac1, depth1), x = sites1[pos]
            (frac2, depth2), y = sites2[pos]
            rows.append('\t'.join(list(pos) + [frac1, depth1, frac2, depth2] + site_values(x, y)) + '\n')
    return ''.join(rows).encode('utf-8', 'surrogateescape'), len(rows)


def _host(bed1, bed2, out, reason):
    global last_compare
    last_compare = None
    data, n_sites = compare_rows(bed1, bed2)
    _write(out, data)
    last_compare = dict(by='host', reason=reason, n_sites=n_sites)
    return n_sites


def compare_by_position(bed1, bed2, xmfa=None, out=None):
    """The host statement: the definition above, one SciPy call after the other.  xmfa is accepted and unused."""
    return _host(bed1, bed2, out, 'the host statement was asked for')


def compare_by_position_device(bed1, bed2, xmfa=None, out=None):
    """The same bytes made on the GPU, or -- when the device declines -- by the host statement, which also words the errors."""
    global last_compare
    from .device import get_device
    last_compare = None
    blob, n_sites, reason = get_device().bed_compare(path1=bed1, path2=bed2)
    if blob is None:
        return _host(bed1, bed2, out, reason)
    _write(out, blob)
    last_compare = dict(by='device', reason=None, n_sites=n_sites)
    return n_sites


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser(description='Compare methylation between two genomes by probabilities of methylation for aligned positions')
    parser.add_argument('--bed1', type=str, required=False, help='bed file 1 with verbose output from make_bed.py')
    parser.add_argument('--bed2', type=str, required=False, help='bed file 2 with verbose output from make_bed.py')
    parser.add_argument('-g', '--genome_alignment', type=str, required=False,
                        help='an xmfa file from mauve (if absent, alignments assumed to be to the same reference genome)')
    parser.add_argument('-o', '--output', type=str, required=False, help='write the rows to this file (default: standard output)')
    parser.add_argument('--device', action='store_true', required=False, help='make the rows on the GPU (the host statement runs when it declines)')
    parser.add_argument('-v', '--version', action='store_true', required=False, help='print version')
    args = parser.parse_args(argv)

    if args.version:
        print('mCallerNP 0.3')
        sys.exit(0)
    if args.bed1 is None or args.bed2 is None:
        parser.error('the following arguments are required: --bed1, --bed2')

    assert os.path.isfile(args.bed1), 'file not found at ' + args.bed1
    assert os.path.isfile(args.bed2), 'file not found at ' + args.bed2

    run = compare_by_position_device if args.device else compare_by_position
    run(args.bed1, args.bed2, args.genome_alignment, args.output)


if __name__ == '__main__':
    main()
