"""phase_reads on the host: the host statement against the brute force of tests/phase_cases.py on the seeded cases and on
written-out lines with every edge of the definition, phi against np.corrcoef, mc_pairphase.h's host build (mc_pair_phi) against the
Python formula bit for bit, nlp against SciPy's fisher_exact, every ValueError, the command line, and the linked bed through
find_motifs."""
import itertools

import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import phase_reads as P
from tests import phase_cases as K


def both(tmp_path, text, fdr=False, threshold=2.0, **opt):
    """The host statement's four results, held against the brute force's."""
    p = K.write(tmp_path, text if isinstance(text, bytes) else text.encode())
    want = K.brute(p, fdr=fdr, threshold=threshold, **opt)
    got = P._rows(p, fdr=fdr, threshold=threshold, want_reads=True, want_bed=True, **opt)
    assert got == want[:4]
    return got


@pytest.mark.parametrize('fdr', [False, True])
@pytest.mark.parametrize('name', sorted(K.DEVICE_CASES) + ['counter_memory', 'many_reads'])
def test_host_statement_is_the_brute_force(tmp_path, name, fdr):
    make = dict(K.DEVICE_CASES, counter_memory=K.case_counter_memory, many_reads=K.case_many_reads)[name]
    text, opt, _ = make()
    rows, reads, bed, fig = both(tmp_path, text, fdr=fdr, threshold=1.0, **opt)
    assert fig['n_pairs'] == rows.count(b'\n') and fig['n_reads'] == reads.count(b'\n') and fig['n_linked'] == bed.count(b'\n')
    assert all(len(r.split(b'\t')) == 11 + fdr for r in rows.splitlines())


def lines_of(calls, chrom='c', strand='+'):
    """calls: [(read, pos, methylated)] in file order"""
    return ''.join(K.row(chrom, read, pos, strand, meth, seven=i % 2 == 1) for i, (read, pos, meth) in enumerate(calls))


OPT1 = dict(depth=1, max_dist=10, min_reads=1, min_margin=1)


def two_sites(table, pos_a=5, pos_b=9, tag='r'):
    """[(read, pos, methylated)] of reads over two sites with the table (n11, n10, n01, n00)."""
    calls, r = [], 0
    for k, (ma, mb) in zip(table, ((True, True), (True, False), (False, True), (False, False))):
        for _ in range(k):
            calls += [('%s%d' % (tag, r), pos_a, ma), ('%s%d' % (tag, r), pos_b, mb)]
            r += 1
    return calls


def test_duplicates_first_wins(tmp_path):
    calls = two_sites((2, 1, 1, 2))
    text = lines_of(calls + [('r0', 5, False), ('r0', 9, False), ('r5', 5, True)])      # r0 was (m, m), r5 was (not, not)
    rows, _, _, fig = both(tmp_path, text, **OPT1)
    assert fig['n_duplicates'] == 3 and rows.split(b'\t')[4:9] == [b'6', b'2', b'1', b'1', b'2']
    # the duplicate does not count towards a site's N either: 6 calls a site, not 7
    assert both(tmp_path, text, **dict(OPT1, depth=7))[3]['n_sites'] == 0 and both(tmp_path, text, **dict(OPT1, depth=6))[3]['n_sites'] == 2


def test_a_site_below_the_depth_between_two_kept(tmp_path):
    calls = two_sites((2, 1, 1, 2), 5, 9) + [('r0', 7, True), ('r1', 7, False)]
    rows, reads, _, fig = both(tmp_path, lines_of(calls), **dict(OPT1, depth=3))
    assert fig['n_sites'] == 2 and [r.split(b'\t')[2:4] for r in rows.splitlines()] == [[b'5', b'9']]
    assert reads.splitlines()[0] == b'c\tr0\t+\t5\t9\t2\t2'                # the call at 7 is at no kept site


def test_strands_and_chroms_do_not_pair(tmp_path):
    text = ''.join(lines_of(two_sites(t, tag=chrom + strand), chrom, strand)
                   for (chrom, strand), t in zip(itertools.product(('x', 'y'), '+-'), ((2, 1, 1, 2), (1, 2, 2, 1), (3, 1, 1, 1), (1, 1, 1, 3))))
    # and one read name on both strands: two read keys
    text += K.row('x', 'x+0', 5, '-', True) + K.row('x', 'x+0', 9, '-', True)
    rows, reads, _, fig = both(tmp_path, text, **OPT1)
    assert fig['n_sites'] == 8 and fig['n_pairs'] == 4 and fig['n_reads'] == 6 + 6 + 6 + 6 + 1
    assert [r.split(b'\t')[:2] + r.split(b'\t')[4:9] for r in rows.splitlines()][1] == [b'x', b'-', b'7', b'2', b'2', b'2', b'1']


def test_pairs_at_and_beyond_max_dist(tmp_path):
    text = lines_of(two_sites((2, 1, 1, 2), 100, 140) + two_sites((2, 1, 1, 2), 300, 341, tag='s'))
    rows, _, _, fig = both(tmp_path, text, **dict(OPT1, max_dist=40))
    assert fig['n_sites'] == 4 and [r.split(b'\t')[2:4] for r in rows.splitlines()] == [[b'100', b'140']]
    assert both(tmp_path, text, **dict(OPT1, max_dist=41))[3]['n_pairs'] == 2 and both(tmp_path, text, **dict(OPT1, max_dist=39))[3]['n_pairs'] == 0


def test_min_reads_and_min_margin_at_equality(tmp_path):
    text = lines_of(two_sites((3, 2, 4, 1)))                            # n = 10; margins 5, 5, 7, 3
    assert both(tmp_path, text, **dict(OPT1, min_reads=10))[3]['n_pairs'] == 1 and both(tmp_path, text, **dict(OPT1, min_reads=11))[3]['n_pairs'] == 0
    assert both(tmp_path, text, **dict(OPT1, min_margin=3))[3]['n_pairs'] == 1 and both(tmp_path, text, **dict(OPT1, min_margin=4))[3]['n_pairs'] == 0
    degenerate = lines_of(two_sites((3, 0, 4, 0)))                      # B is methylated on every read: a margin of 0
    assert both(tmp_path, degenerate, **OPT1)[3]['n_pairs'] == 0


def test_a_read_whose_rows_lie_apart_and_the_order_of_the_rows(tmp_path):
    """Sites first seen in the order 9, 5, 7: rows by A's first row, within A by posB; a read's rows far apart in the file and out of
    position order; equal ints under two texts ('7' and '07') are two sites that never pair with each other."""
    calls = [('r0', 9, True), ('r1', 5, False), ('r2', 7, True), ('r3', '07', True)]
    calls += [('r%d' % r, pos, (r + pos) % 3 == 0) for pos in (5, 7, 9) for r in range(4, 12)]
    calls += [('r0', 5, True), ('r1', 9, False), ('r2', 5, False), ('r0', 7, False), ('r3', 5, True), ('r3', 9, True), ('r4', '07', True), ('r5', '07', False)]
    rows, reads, _, fig = both(tmp_path, lines_of(calls), **OPT1)
    assert [tuple(r.split(b'\t')[2:4]) for r in rows.splitlines()] == [(b'5', b'7'), (b'5', b'07'), (b'5', b'9'), (b'7', b'9'), (b'07', b'9')]
    assert reads.splitlines()[0] == b'c\tr0\t+\t5\t9\t3\t2' and fig['n_sites'] == 4


def test_phi_is_the_correlation_of_the_two_vectors():
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(2000):
        t = [int(v) for v in rng.integers(0, 40, size=4)]
        if min(t[0] + t[1], t[2] + t[3], t[0] + t[2], t[1] + t[3]) < 1:
            continue
        a = np.repeat([1.0, 1.0, 0.0, 0.0], t)
        b = np.repeat([1.0, 0.0, 1.0, 0.0], t)
        worst = max(worst, abs(P.phi_of(*t) - np.corrcoef(a, b)[0, 1]))
    print('largest difference of phi to np.corrcoef: %.3g' % worst)
    assert worst <= 1e-12                                                # fewer than ten roundings on a value in [-1, 1]


def test_pair_phi_has_the_formulas_bits():
    tables = [t for t in itertools.product(range(13), repeat=4) if sum(t) <= 12]
    rng = np.random.default_rng(7)
    tables += [tuple(int(v) for v in rng.integers(0, 65536, size=4)) for _ in range(10000)]
    tables += [(65535,) * 4, (65535, 0, 0, 65535), (1, 65535, 65535, 1)]
    n = 0
    for t in tables:
        got = _lib.pair_phi(*t)
        if min(t[0] + t[1], t[2] + t[3], t[0] + t[2], t[1] + t[3]) < 1:
            assert got is None, t
            continue
        phi = P.phi_of(*t)
        assert got[0].hex() == phi.hex() and np.float64(got[1]).hex() == float(np.round(phi, 3)).hex() and str(np.float64(got[1])) == str(np.round(phi, 3)), t
        n += 1
    assert n > 10000 and _lib.pair_phi(1, 0, 0, 1) == (1.0, 1.0) and _lib.pair_phi(0, 1, 1, 0) == (-1.0, -1.0)
    with pytest.raises(ValueError):
        _lib.pair_phi(65536, 1, 1, 1)


def test_nlp_against_scipy(tmp_path):
    from scipy.stats import fisher_exact
    text, opt, _ = K.case_shuffled()
    written = K.brute(K.write(tmp_path, text), **opt)[4]
    worst = 0.0
    for (n11, n10, n01, n00), L in written:
        want = fisher_exact([[n11, n10], [n01, n00]])[1]
        worst = max(worst, abs(10.0 ** L - want) / want)
    print('largest relative difference of p to SciPy over %d tables: %.3g' % (len(written), worst))
    assert len(written) > 100 and worst <= 1e-12                        # tests/test_fisher_bh.py's tolerance for this comparison


def test_every_value_error(tmp_path):
    good = K.row('c', 'r', 5, '+', True)
    for bad, message in ((good + 'c\tr\t5\n', 'line 2: 3 tab-separated fields'),
                         (good + good.replace('0.5,', '0.5x,'), 'line 2: a value that is no number'),
                         (good + good.replace('0.5,', '0.5,0.25,'), 'line 2: 3 values, 2 are expected'),
                         (good.replace('0.5,', ''), 'line 1: 1 values, at least 2 are needed'),
                         (good + good.replace('\t5\t', '\t5x\t'), 'line 2: a position that is no integer'),
                         (good.replace('0.5,', 'x,').replace('\t5\t', '\tx\t') + 'c\n', 'line 1: a value that is no number')):
        p = K.write(tmp_path, bad.encode())
        with pytest.raises(ValueError, match=message):
            P.phase_reads(p, out=str(tmp_path / 'o'))
    p = K.write(tmp_path, good.encode())
    for kw, message in ((dict(depth=0), '-d is at least 1'), (dict(max_dist=0), '--max_dist is at least 1'), (dict(min_reads=0), '--min_reads is at least 1'),
                        (dict(min_margin=0), '--min_margin is at least 1'), (dict(threshold=float('nan')), '--threshold is a number')):
        with pytest.raises(ValueError, match=message):
            P.phase_reads(p, out=str(tmp_path / 'o'), **kw)
    assert P.phase_reads(K.write(tmp_path, good.replace('\t5\t', '\t+5\t').encode()), out=str(tmp_path / 'o')) == 0      # int() takes it


def test_the_command_line_and_find_motifs(tmp_path, capsys):
    from mcaller_amd import find_motifs as FM
    text, opt, _ = K.case_shuffled()
    p = K.write(tmp_path, text)
    want, want_reads, want_bed, fig = P._rows(p, fdr=True, threshold=0.5, want_reads=True, want_bed=True, **opt)
    out, reads, bed = (str(tmp_path / n) for n in ('o.tsv', 'o.reads', 'o.bed'))
    P.main(['-f', p, '-d', '10', '--max_dist', '50', '--min_reads', '10', '--min_margin', '2', '--fdr', '--reads', reads, '--linked_bed', bed,
            '--threshold', '0.5', '-o', out])
    assert (open(out, 'rb').read(), open(reads, 'rb').read(), open(bed, 'rb').read()) == (want, want_reads, want_bed)
    assert P.last_phase == dict(by='host', reason='the host statement was asked for', **fig) and 0 < fig['n_linked'] < fig['n_sites']
    P.main(['-f', p, '-d', '10', '--max_dist', '50'])
    assert capsys.readouterr().out.encode() == P._rows(p, depth=10, max_dist=50)[0]
    with pytest.raises(SystemExit):
        P.main(['-f', p, '--min_margin', '0'])
    lines = want_bed.decode().splitlines()
    assert all(len(l.split('\t')) == 7 and int(l.split('\t')[4]) > 0 and l.split('\t')[6] == '14' for l in lines)
    listed = FM.read_sites(bed, {'chr1': 'A' * 600})
    assert int(listed['chr1'][0].sum() + listed['chr1'][1].sum()) == len(lines) == fig['n_linked']
