#!/usr/bin/env python3
"""How good are the calls of a `.diffs.<k>` file, and which `-d` / `-t` should make_bed run with?  ROC tables by read, by site
and by site at subsampled depth, against a labelled positions file:

    python -m mcaller_amd.evaluate -f reads.eventalign.diffs.6 -p labelled_positions.txt [-d 15] [--depths 1,2,5,10,15,20,30,50] [-o OUT] [--device]

The reference prints cross-validation accuracy at --train and nothing else; the curves of the paper behind it (per read, per
site, per site at subsampled coverage) have no code there.  This module is their definition here: `evaluate_calls` is the host
statement, plain Python / NumPy with exact rationals, deterministic -- the paper's random subsampling of reads is replaced by its
expectation, so there is no RNG.  The default output is `<-f>.split('.')[0] + '.evaluation.tsv'`, make_bed's naming rule.

Truth.  The -p file as mCaller.pos2label reads it: split on '\\n', keep lines with more than one whitespace token, key
(tok[0], int(tok[1]), tok[2]), value tok[3], the last line of a key wins; a kept line with fewer than four tokens raises
(IndexError, as there).  A site is POSITIVE when its label starts with 'm'.

Rows.  Every `.diffs` line split on '\\t' has eight fields, or ValueError names the line.  A row whose context has no 'M' at
len // 2 is skipped (n_not_m); a row whose (chrom, int(pos), strand) is not in the truth is skipped (n_unlabelled).  Of a kept
row the call is "methylated" when its label field starts with 'm', the score is float(prob.strip()); a score outside [0, 1] or
nan raises.  A site is (chrom, pos, strand) -- the context is no part of the key; N its kept rows, K those called methylated.

Thresholds.  thr[j] = j / 100 in fp64, j = 0 .. 100; every comparison against one is the fp64 `>=`.

Tables, 101 rows each:
  read      over kept rows, the score the probability; TP and FP integers
  site all  over sites with N >= min_depth, the score K / N (one fp64 division: np.mean of make_bed's 0/1 list)
  site d    for each d of --depths (up to 16, each 1 .. 1024, strictly increasing): over sites with N >= d, whatever min_depth
            is.  k_min(d, j) is the smallest x in 0 .. d + 1 with x == d + 1 or x / d >= thr[j] (the fp64 comparison
            is make_bed's; both quotients are correctly rounded, so up to d = 1024 it decides as the rationals do).  A site contributes T = P(X >= k_min), X ~ Hypergeometric(N, K, d):
            draw d of its N reads without replacement.  E_TP[d][j] sums T over positive sites, E_FP over negative ones -- as
            exact Fractions, converted to float once.

Rates and AUC.  tpr = TP / P, fpr = FP / N_neg (E_TP / P_d, E_FP / N_d); nan when the class is empty.  The AUC is the trapezoid
over the 101 points and a closing point (0, 0): sum_j (FP_j - FP_{j+1})(TP_j + TP_{j+1}) / (2 P N_neg) as Python's integer
quotient (correctly rounded); for the expected tables the same sum over exact rates.  Every rate and AUC is printed as
str(np.round(v, 4)).  mCaller prints probabilities as str(np.round(p, 2)), so on its own files the `read` AUC is the exact
Mann-Whitney AUC with ties.

Bytes.  '#level\\tdepth\\tthreshold\\tn_pos\\tn_neg\\ttp\\tfp\\ttpr\\tfpr', then the rows 'read\\t-\\t..', 'site\\tall\\t..',
'site\\t<d>\\t..' in the order of --depths (tp and fp are '-' there), the threshold as repr(j / 100); then 'auc\\tread\\t-\\t<v>',
'auc\\tsite\\tall\\t<v>', 'auc\\tsite\\t<d>\\t<v>'.

`last_eval` records what the last call did, in the style of make_bed.last_summary.  Without --device the tables are made on the host
and no GPU is touched.  --device makes the file on the GPU (csrc/eval/mc_evalcalls.hip; evaluate_calls_device): the text of both
files -> kernels -> these bytes, or a decline -- wherever the host would raise, wherever the device reader is not sure it reads
what Python reads, and wherever an expected value's DERIVED error bound reaches a tie of np.round(., 4) -- which main says on stderr
before it runs the host statement (last_eval['by'] is 'device' or 'host', last_eval['reason'] the decline).  The arithmetic of the
"site d" tables on the device is csrc/mc_hypergeom.h, built for the host and the device: all 101 tails of a (N, K, d) from one pair of
walks with one bound (_lib.hypergeom_masses, Device.hypergeom_masses), the single tail (_lib.hypergeom_tail), np.round(., 4)
restated, the tie test."""
import argparse
import io
import math
import sys
from fractions import Fraction

import numpy as np

DEFAULT_DEPTHS = (1, 2, 5, 10, 15, 20, 30, 50)
MAX_DEPTHS = 16
MAX_DEPTH = 1024
N_THR = 101
HEADER = '#level\tdepth\tthreshold\tn_pos\tn_neg\ttp\tfp\ttpr\tfpr'

# what the last evaluate_calls did
last_eval = dict(by=None, reason=None, n_rows=0, n_kept=0, n_unlabelled=0, n_not_m=0, n_sites=0, n_pos_sites=0, n_neg_sites=0)


def thresholds():
    return [j / 100 for j in range(N_THR)]


def _text(source):
    """A path (str / PathLike) or the file's bytes -> its text as open(path, 'r') reads it."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return io.TextIOWrapper(io.BytesIO(bytes(source))).read()
    with open(source, 'r') as fh:
        return fh.read()


def read_truth(positions):
    """mCaller.pos2label's dict: (chrom, int(pos), strand) -> label."""
    return {(pos.split()[0], int(pos.split()[1]), pos.split()[2]): pos.split()[3]
            for pos in _text(positions).split('\n') if len(pos.split()) > 1}


def check_depths(depths):
    depths = [int(d) for d in depths]
    if len(depths) > MAX_DEPTHS:
        raise ValueError('--depths: at most %d depths' % MAX_DEPTHS)
    if any(d < 1 or d > MAX_DEPTH for d in depths) or any(b <= a for a, b in zip(depths, depths[1:])):
        raise ValueError('--depths: each from 1 to %d, strictly increasing' % MAX_DEPTH)
    return depths


def k_min(d):
    """k_min(d, j) for j = 0 .. 100: the smallest x in 0 .. d + 1 with x == d + 1 or x / d >= thr[j], the division in fp64."""
    out, x = [], 0
    for t in thresholds():                                 # thr rises with j, so x only moves up
        while x <= d and not x / d >= t:
            x += 1
        out.append(x)
    return out


def tail_numerators(N, K, d):
    """-> (num[0 .. d + 1], den): P(X >= x) = num[x] / den exactly, X ~ Hypergeometric(N, K, d)."""
    num = [0] * (d + 2)
    for x in range(min(K, d), -1, -1):
        num[x] = num[x + 1] + math.comb(K, x) * math.comb(N - K, d - x)
    return num, math.comb(N, d)


def _counts_at_least(scores):
    """[#(score >= thr[j]) for j]: the fp64 comparison, by a sort."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    return [int(len(s) - np.searchsorted(s, t, side='left')) for t in thresholds()]


def _exact_rate(a, n):
    """a / n as a Fraction (a an int or a Fraction), None for an empty class."""
    return Fraction(a) / n if n else None


def _exact_auc(tp, fp, P, Nn):
    """The trapezoid over the 101 points and the closing point (0, 0) as a Fraction; tp / fp ints or Fractions."""
    if not P or not Nn:
        return None
    tp, fp = list(tp) + [0], list(fp) + [0]
    return Fraction(sum((fp[j] - fp[j + 1]) * (tp[j] + tp[j + 1]) for j in range(N_THR))) / (2 * P * Nn)


def _float(fr):
    """An exact value correctly rounded (for two integers what Python's integer quotient gives), nan for None."""
    return float('nan') if fr is None else float(fr)


def _table(level, depth, P, Nn, tp, fp, integers):
    tpr, fpr, auc = [_exact_rate(v, P) for v in tp], [_exact_rate(v, Nn) for v in fp], _exact_auc(tp, fp, P, Nn)
    return dict(level=level, depth=depth, n_pos=P, n_neg=Nn, tp=tp if integers else None, fp=fp if integers else None,
                tpr=[_float(v) for v in tpr], fpr=[_float(v) for v in fpr], auc=_float(auc), exact=tpr + fpr + [auc])


def _num(v):
    return str(np.round(np.float64(v), 4))


def evaluate_tables(diffs, positions, min_depth=15, depths=DEFAULT_DEPTHS):
    """The tables before they are printed: a list of dict(level=, depth=, n_pos=, n_neg=, tp=, fp=, tpr=, fpr=, auc=, exact=) --
    'read', 'site' 'all', then 'site' d per depth; tp / fp lists of 101 ints (None in the expected tables), tpr / fpr lists of 101
    floats, auc a float, none of them rounded yet; exact: the 203 printed values as Fractions (None: nan).  Fills last_eval."""
    depths = check_depths(depths)
    min_depth = int(min_depth)
    truth = read_truth(positions)
    sites = {}                                              # (chrom, pos, strand) -> [N, K], in first-occurrence order
    scores = ([], [])                                       # kept rows' probabilities: of negative, of positive sites
    n_rows = n_not_m = n_unlabelled = 0
    for lineno, line in enumerate(io.StringIO(_text(diffs)), 1):
        n_rows += 1
        f = line.split('\t')
        if len(f) != 8:
            raise ValueError('line %d: not eight tab-separated fields: %r' % (lineno, line[:80]))
        chrom, pos, context, strand, label, prob = f[0], f[2], f[3], f[5], f[6], f[7]
        if context[len(context) // 2] != 'M':
            n_not_m += 1
            continue
        key = (chrom, int(pos), strand)
        if key not in truth:
            n_unlabelled += 1
            continue
        p = float(prob.strip())
        if not 0.0 <= p <= 1.0:                             # (nan too)
            raise ValueError('line %d: a probability outside [0, 1]: %r' % (lineno, prob.strip()))
        nk = sites.setdefault(key, [0, 0])
        nk[0] += 1
        nk[1] += 1 if label.startswith('m') else 0
        scores[1 if truth[key].startswith('m') else 0].append(p)
    positive = {key: truth[key].startswith('m') for key in sites}
    tables = []

    def integer_table(level, depth, sc_neg, sc_pos):
        P, Nn = len(sc_pos), len(sc_neg)
        tp, fp = _counts_at_least(sc_pos), _counts_at_least(sc_neg)
        tables.append(_table(level, depth, P, Nn, tp, fp, True))

    integer_table('read', '-', scores[0], scores[1])
    deep = [key for key, (N, K) in sites.items() if N >= min_depth]
    integer_table('site', 'all', [np.float64(sites[k][1]) / np.float64(sites[k][0]) for k in deep if not positive[k]],
                  [np.float64(sites[k][1]) / np.float64(sites[k][0]) for k in deep if positive[k]])
    for d in depths:
        km = k_min(d)
        shapes = ({}, {})                                   # per class: N -> {K: sites}
        for key, (N, K) in sites.items():
            if N >= d:
                by_K = shapes[1 if positive[key] else 0].setdefault(N, {})
                by_K[K] = by_K.get(K, 0) + 1
        expected, n_class = [], []
        for cls in (0, 1):
            e = [Fraction(0)] * N_THR
            n_class.append(sum(sum(by_K.values()) for by_K in shapes[cls].values()))
            for N, by_K in shapes[cls].items():             # sites of one N share the denominator C(N, d)
                top = [0] * N_THR
                den = 1
                for K, count in by_K.items():
                    num, den = tail_numerators(N, K, d)
                    for j in range(N_THR):
                        top[j] += count * num[km[j]]
                for j in range(N_THR):
                    e[j] += Fraction(top[j], den)
            expected.append(e)
        (e_fp, e_tp), (Nn, P) = expected, n_class
        tables.append(_table('site', str(d), P, Nn, e_tp, e_fp, False))
    last_eval.update(by='host', reason=None, n_rows=n_rows, n_kept=n_rows - n_not_m - n_unlabelled, n_unlabelled=n_unlabelled, n_not_m=n_not_m,
                     n_sites=len(sites), n_pos_sites=sum(positive.values()), n_neg_sites=len(sites) - sum(positive.values()))
    return tables


def evaluate_calls(diffs, positions, min_depth=15, depths=DEFAULT_DEPTHS):
    """The host statement: the evaluation of the `.diffs` rows (a path, or the file's bytes) against the labelled positions
    (a path, or bytes) -> the bytes of the evaluation file.  Fills last_eval."""
    thr = thresholds()
    lines, aucs = [HEADER], []
    for t in evaluate_tables(diffs, positions, min_depth, depths):
        for j in range(N_THR):
            counts = '%d\t%d' % (t['tp'][j], t['fp'][j]) if t['tp'] is not None else '-\t-'
            lines.append('%s\t%s\t%r\t%d\t%d\t%s\t%s\t%s' % (t['level'], t['depth'], thr[j], t['n_pos'], t['n_neg'], counts, _num(t['tpr'][j]), _num(t['fpr'][j])))
        aucs.append('auc\t%s\t%s\t%s' % (t['level'], t['depth'], _num(t['auc'])))
    return ('\n'.join(lines + aucs) + '\n').encode('ascii')


def evaluate_calls_device(diffs, positions, min_depth=15, depths=DEFAULT_DEPTHS, device=None):
    """evaluate_calls on the GPU (csrc/eval/mc_evalcalls.hip; `device`: a Device, default the process's): the same bytes, or None
    when the device declines -- last_eval['reason'] says why, and the caller runs evaluate_calls.  Fills last_eval from the
    device's figures (by='device') when it served the call.  No GPU: the error of the device's creation, never a host run."""
    from .device import get_device
    depths = check_depths(depths)
    dev = device if device is not None else get_device()
    is_text = lambda s: isinstance(s, (bytes, bytearray, memoryview))
    kw = dict(text=bytes(diffs)) if is_text(diffs) else dict(path=diffs)
    kw.update(dict(positions_text=bytes(positions)) if is_text(positions) else dict(positions_path=positions))
    data, reason = dev.eval_calls(min_depth=int(min_depth), depths=depths, **kw)
    if data is None:
        last_eval.update(by=None, reason=reason)
        return None
    s = dev.eval_calls_last_stats()
    last_eval.update(by='device', reason=None, n_rows=int(s['n_rows']), n_kept=int(s['n_kept']), n_unlabelled=int(s['n_unlabelled']),
                     n_not_m=int(s['n_not_m']), n_sites=int(s['n_sites']), n_pos_sites=int(s['n_pos_sites']), n_neg_sites=int(s['n_neg_sites']))
    return data


def default_output(diffs_path):
    return diffs_path.split('.')[0] + '.evaluation.tsv'


def main(argv=None):
    ap = argparse.ArgumentParser(description='ROC tables of mCaller calls by read, by site and by site at subsampled depth')
    ap.add_argument('-f', '--file', required=True, help='the .diffs.<k> file of a predict run over the labelled positions')
    ap.add_argument('-p', '--positions', required=True, help='the labelled positions file: chrom, position, strand, label')
    ap.add_argument('-d', '--min_read_depth', type=int, default=15, help='least depth of a site of the "site all" table (default 15)')
    ap.add_argument('--depths', default=','.join(str(d) for d in DEFAULT_DEPTHS), help='subsampled depths, comma-separated, increasing')
    ap.add_argument('-o', '--output', default=None, help='output file (default: <-f up to its first dot>.evaluation.tsv)')
    ap.add_argument('--device', action='store_true', help='make the file on the GPU; where the device declines, say so and run the host statement')
    args = ap.parse_args(argv)
    depths = check_depths(int(x) for x in args.depths.split(',') if x.strip())
    out = args.output or default_output(args.file)
    data = evaluate_calls_device(args.file, args.positions, args.min_read_depth, depths) if args.device else None
    if data is None:
        reason = last_eval['reason'] if args.device else None
        if args.device:
            print('%s: %s; the host statement makes the file' % (args.file, reason), file=sys.stderr)
        data = evaluate_calls(args.file, args.positions, args.min_read_depth, depths)
        last_eval['reason'] = reason
    with open(out, 'wb') as fh:
        fh.write(data)
    print('%s: %d rows, %d kept (%d unlabelled, %d without a centre M), %d sites (%d positive, %d negative)' % (
        out, last_eval['n_rows'], last_eval['n_kept'], last_eval['n_unlabelled'], last_eval['n_not_m'], last_eval['n_sites'],
        last_eval['n_pos_sites'], last_eval['n_neg_sites']), file=sys.stderr)
    return out


if __name__ == '__main__':
    main()
