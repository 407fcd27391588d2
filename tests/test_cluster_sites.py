"""cluster_sites without a GPU: the host statement (mcaller_amd/cluster_sites.py) against the brute force of its definition
(tests/cluster_cases.py), against SciPy's complete linkage where no two distances are equal, the adjusted Rand index against
scikit-learn, the C++ rule (csrc/mc_linkage.h, host build) against the host statement bit for bit, and the entry points."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import cluster_sites as CS
from tests import cluster_cases as K
from tests import helpers as H

METRICS = ('correlation', 'euclidean')


def host_is_brute(tmp_path, text, what='', **kw):
    p = K.write(tmp_path, text)
    rows, bed, n, n_mixed = CS._rows(p, kw.get('depth', 15), kw.get('max_depth', 256), kw.get('metric', 'correlation'), kw.get('mixed', False),
                                     kw.get('min_minor', 0.2), kw.get('min_gap', 2.0))
    want, want_bed = K.brute_rows(text, **kw)
    assert rows == want and (bed or b'') == want_bed, what
    assert n == want.count(b'\n') and n_mixed == want_bed.count(b'\n')
    return rows, bed, n


@pytest.mark.parametrize('metric', METRICS)
def test_random_sites(tmp_path, metric):
    text = K.seeded_text(24, 3, 40, seed=3)
    rows, bed, n = host_is_brute(tmp_path, text, depth=5, metric=metric, mixed=True, min_gap=1.3)
    assert 15 <= n <= 24 and 0 < bed.count(b'\n') < n
    first = rows.decode().splitlines()[0].split('\t')
    assert len(first) == 14 and int(first[2]) == int(first[1]) + 1 and int(first[7]) + int(first[8]) == int(first[5]) - int(first[6])


@pytest.mark.parametrize('metric', METRICS)
def test_duplicated_and_identical_rows(tmp_path, metric):
    rng = np.random.default_rng(11)
    X = K.gaussian(rng, 7)
    dup = np.vstack([X, X[2], X[2], X[5], X])                          # rows at distance 0.0 of each other
    same = np.tile(K.gaussian(rng, 1), (9, 1))                         # every distance equal: the index rule decides every merge
    text = K.text_of([K.site_lines('c', 5, '+', dup), K.site_lines('c', 9, '-', same)])
    rows, _, n = host_is_brute(tmp_path, text, depth=2, metric=metric)
    assert n == 2
    f = rows.decode().splitlines()[1].split('\t')
    assert f[7:9] == ['8', '1'] and float(f[11]) <= 1e-15 and f[12] == '0.0'      # rows 0 .. 7 merge first, one by one, into cluster 1


@pytest.mark.parametrize('metric', METRICS)
def test_small_integers_tie_all_the_time(tmp_path, metric):
    text = K.seeded_text(30, 4, 18, seed=17, c=3, maker=K.integers, planted=0)
    host_is_brute(tmp_path, text, depth=3, metric=metric, mixed=True, min_gap=1.0)
    ties = 0
    rng = np.random.default_rng(5)
    for _ in range(10):
        got = K.brute_split(K.integers(rng, 12, 3), metric)
        ties += got is not None and len(set(got[4])) < len(got[4])
    assert ties >= 8


def test_flat_rows(tmp_path):
    """Constant rows are flat under correlation: left out, counted in n_flat, and the anchor of cluster 1 moves to the first usable
    row; under euclidean they are rows like any other.  A site of flat rows alone is not kept."""
    rng = np.random.default_rng(23)
    X = np.vstack([np.full((2, 6), 0.5), K.gaussian(rng, 6, split=3.0), np.full((1, 6), -2.0)])
    text = K.text_of([K.site_lines('c', 5, '+', X), K.site_lines('c', 8, '+', np.full((5, 6), 1.0))])
    rows, _, n = host_is_brute(tmp_path, text, depth=3)
    f = rows.decode().splitlines()[0].split('\t')
    assert n == 1 and f[5:7] == ['9', '3'] and int(f[7]) + int(f[8]) == 6
    rows, _, n = host_is_brute(tmp_path, text, depth=3, metric='euclidean')
    assert n == 2 and [r.split('\t')[6] for r in rows.decode().splitlines()] == ['0', '0']
    assert host_is_brute(tmp_path, text, depth=7)[2] == 0              # six usable rows are fewer than -d


def test_two_usable_rows(tmp_path):
    text = K.text_of([K.site_lines('c', 5, '+', [[1.0, 2.0, 4.0], [3.0, 1.0, 0.0], [2.0, 2.0, 2.0]])])
    rows, _, n = host_is_brute(tmp_path, text, depth=2)
    f = rows.decode().splitlines()[0].split('\t')
    assert n == 1 and f[5:9] == ['3', '1', '1', '1'] and f[12] == '0.0' and float(f[11]) > 1.0


def test_max_depth_cut(tmp_path):
    """n = max_depth and n = max_depth + 1: the later row is counted in n and changes nothing else."""
    rng = np.random.default_rng(29)
    X = K.gaussian(rng, 13, split=2.0)
    at, over = K.text_of([K.site_lines('c', 5, '+', X[:12])]), K.text_of([K.site_lines('c', 5, '+', X)])
    a = host_is_brute(tmp_path, at, depth=4, max_depth=12)[0].decode().split('\t')
    b = host_is_brute(tmp_path, over, depth=4, max_depth=12)[0].decode().split('\t')
    assert (a[5], b[5]) == ('12', '13') and a[6:] == b[6:]
    c = host_is_brute(tmp_path, over, depth=4, max_depth=13)[0].decode().split('\t')
    assert c[5] == '13' and int(c[7]) + int(c[8]) == 13


@pytest.mark.parametrize('fields', [7, 8, 'mixed'])
def test_seven_and_eight_fields(tmp_path, fields):
    rng = np.random.default_rng(31)
    text = K.text_of([K.site_lines('c', 5, '+', K.gaussian(rng, 9, split=2.0), fields=fields)])
    rows, _, n = host_is_brute(tmp_path, text, depth=3)
    assert n == 1 and int(rows.decode().split('\t')[9]) + int(rows.decode().split('\t')[10]) == 3      # the methylated rows: every third


def test_every_value_error(tmp_path):
    good = K.site_lines('c', 5, '+', [[1.0, 2.0, 4.0], [3.0, 1.0, 0.0]])
    def fails(lines, match, **kw):
        with pytest.raises(ValueError, match=match):
            CS.cluster_sites(K.write(tmp_path, ''.join(lines).encode()), out=str(tmp_path / 'o'), **kw)
    fails(good + ['c\tr\t5\n'], 'line 3: 3 tab-separated fields')
    fails(good + [good[0].replace('1.0,', 'x,')], 'line 3: a value that is no number')
    fails(good + [good[0].replace('1.0,', '')], 'line 3: 3 values, 4 are expected')
    fails([good[0].replace('1.0,2.0,', '')], 'line 1: 2 values, at least 3 are needed')
    fails(good + [good[0].replace('1.0,', 'inf,')], 'line 3: a value that is not finite')
    fails(good + [good[0].replace('1.0,', 'nan,')], 'line 3: a value that is not finite')
    fails(good + [good[0].replace('\t5\t', '\t5.5\t')], 'line 3: a position that is no integer')
    fails(good, '-d is at least 2', depth=1)
    fails(good, '--max_depth is 2 to 1024', max_depth=1025)
    fails(good, '--max_depth is 2 to 1024', max_depth=1)
    fails(good, '--metric', metric='cosine')


@pytest.mark.parametrize('metric', METRICS)
def test_against_scipy_where_nothing_ties(metric):
    """fcluster(linkage(pdist(X), 'complete'), 2, 'maxclust') relabelled so that cluster 1 holds row 0; the distances against pdist.
    (No site of c = 2: under correlation every u is then +-(1, -1) / sqrt(2) and all distances are 0 or 2.)"""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import pdist, squareform
    rng = np.random.default_rng(41)
    for n, c in [(2, 6), (3, 6), (5, 3), (17, 6), (40, 7), (64, 6), (65, 6), (150, 6)]:
        X = rng.normal(0.0, 1.0, size=(n, c))
        U, keep = CS.usable_rows(X, metric)
        assert len(keep) == n
        D = CS.distances(U, metric)
        mine = D[np.triu_indices(n, 1)]
        assert len(set(mine.tolist())) == len(mine), 'two pair distances of the site are equal'
        theirs = pdist(X, metric)
        assert np.max(np.abs(mine - theirs)) <= 1e-12 and np.array_equal(D, D.T)
        labels, h_top, h_sub = CS.link_two(D)
        Z = linkage(theirs, 'complete')
        ref = fcluster(Z, 2, 'maxclust')
        ref = np.where(ref == ref[0], 1, 2)
        assert np.array_equal(labels, ref), (n, c)
        assert abs(h_top - Z[-1, 2]) <= 1e-12
        if n > 2:
            below = [Z[int(k) - n, 2] if k >= n else 0.0 for k in Z[-1, :2]]
            assert abs(h_sub - max(below)) <= 1e-12
        else:
            assert h_sub == 0.0
        assert abs(h_top - np.max(squareform(theirs)[np.ix_(labels == 1, labels == 2)])) <= 1e-12


def test_ari_against_sklearn_over_every_table():
    from sklearn.metrics import adjusted_rand_score
    count = 0
    for n in range(2, 13):
        for n1 in range(1, n):
            n2 = n - n1
            for m1, m2 in itertools.product(range(n1 + 1), range(n2 + 1)):
                cluster = [1] * n1 + [2] * n2
                meth = [1] * m1 + [0] * (n1 - m1) + [1] * m2 + [0] * (n2 - m2)
                want = adjusted_rand_score(meth, cluster)
                got = CS.ari_of(n1, n2, m1, m2)
                assert abs(got - want) <= 1e-12, (n1, n2, m1, m2)
                assert got == K.brute_ari(cluster, meth) == _lib.site_ari(n1, n2, m1, m2)
                count += 1
    assert count > 1000
    big = CS.ari_of(512, 512, 256, 256), CS.ari_of(1, 1023, 1, 0), CS.ari_of(700, 324, 700, 0)
    assert big == (_lib.site_ari(512, 512, 256, 256), _lib.site_ari(1, 1023, 1, 0), _lib.site_ari(700, 324, 700, 0)) and big[2] == 1.0


@pytest.mark.parametrize('metric', METRICS)
def test_the_cpp_rule_is_the_host_statement(metric):
    """mc_site_cluster_host == site_split: labels equal, heights bit for bit -- Gaussian sites, tie-ridden integer sites, duplicated
    and identical rows, flat rows in front."""
    rng = np.random.default_rng(43)
    sites = [K.gaussian(rng, n, c, split) for n, c, split in [(2, 6, 0.0), (3, 2, 0.0), (20, 6, 2.0), (63, 6, 0.0), (64, 7, 1.0), (65, 6, 0.0), (200, 3, 1.0)]]
    sites += [K.integers(rng, n, 3) for n in (4, 9, 30, 70)]
    sites += [np.tile(K.gaussian(rng, 1), (11, 1)), np.vstack([np.full((3, 6), 2.0), K.gaussian(rng, 8), np.full((1, 6), 0.0)])]
    sites += [np.vstack([X, X]) for X in (K.gaussian(rng, 6), K.integers(rng, 5, 2))]
    seen_tie = False
    for X in sites:
        meth = np.arange(len(X)) % 2 == 0
        want = CS.site_split(X, meth, metric)
        got = _lib.site_cluster(X, metric)
        if want is None:
            assert got is None
            continue
        labels, h_top, h_sub = got
        assert np.array_equal(labels[labels > 0], want[8]) and int(np.sum(labels == 0)) == want[0]
        assert (h_top, h_sub) == (want[5], want[6]), (X.shape, h_top, want[5])
        brute = K.brute_split(X, metric)
        assert brute[1] == list(want[8]) and (brute[2], brute[3]) == (h_top, h_sub)
        seen_tie = seen_tie or len(set(brute[4])) < len(brute[4])
    assert seen_tie
    assert _lib.site_cluster(np.full((4, 3), 1.0), 'correlation') is None
    with pytest.raises(ValueError):
        _lib.site_cluster(np.zeros((2, 1)), metric)


def test_make_bed_plot_still_raises(tmp_path):
    from mcaller_amd import make_bed
    p = K.write(tmp_path, K.seeded_text(2, 3, 4, seed=1))
    with pytest.raises(NotImplementedError):
        make_bed.main(['-f', p, '--plot'])


def test_the_script_writes_what_the_function_writes(tmp_path):
    text = K.seeded_text(12, 6, 20, seed=47)
    p = K.write(tmp_path, text)
    out, bed, out2, bed2 = (str(tmp_path / n) for n in ('o.tsv', 'o.bed', 'f.tsv', 'f.bed'))
    n = CS.cluster_sites(p, out=out2, depth=6, max_depth=16, metric='euclidean', mixed_bed=bed2, min_minor=0.1, min_gap=1.2)
    assert CS.last_cluster == dict(by='host', reason='the host statement was asked for', n_sites=n, n_mixed=open(bed2, 'rb').read().count(b'\n'))
    subprocess.check_call([sys.executable, os.path.join(H.REPO, 'cluster_sites.py'), '-f', p, '-d', '6', '--max_depth', '16', '--metric', 'euclidean',
                           '--mixed_bed', bed, '--min_minor', '0.1', '--min_gap', '1.2', '-o', out])
    assert open(out, 'rb').read() == open(out2, 'rb').read() != b'' and open(bed, 'rb').read() == open(bed2, 'rb').read()
    assert n == 12 and open(out, 'rb').read() == K.brute_rows(text, depth=6, max_depth=16, metric='euclidean')[0]
