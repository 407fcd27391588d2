"""Every case of tests/forest_fit_cases.py reaches the path of k5_forest_fit / k5_forest_val it is there for -- shown WITHOUT a GPU,
on the trees of tests/forest_fit_oracle.py alone (never on the device's: tests/test_gpu_forest_fit_edges.py holds those against the
same trees).  A case that stops reaching its path fails here."""
import numpy as np
import pytest

from tests import forest_fit_cases as FC

BT = FC.BT


def trees_of(name, job=0):
    return FC.oracle(name)[job]['trees']


def chunks_with_splits(level):
    nodes, pos = level
    return sorted(set(int(p) // BT for p in pos))


def test_levels_gives_the_level_order_of_a_small_tree():
    # pre-order: 0 (1 (2, 3 (4, 5)), 6)
    tree = dict(left=np.array([1, 2, -1, 4, -1, -1, -1]), right=np.array([6, 3, -1, 5, -1, -1, -1]))
    lv = FC.levels(tree)
    assert [list(n) for n, _ in lv] == [[0], [1, 6], [2, 3], [4, 5]]
    assert [list(p) for _, p in lv] == [[0], [0], [1], []]
    assert FC.widest(tree) == (2, 0)


def test_two_chunks_a_level_splits_in_its_first_and_in_its_second_chunk():
    """A split node at level position >= 256 takes its rank and the start of its left rows from the sums of the first chunk; a
    split node before it in the same level makes those sums more than zero."""
    hits = [lv for tr in trees_of('two_chunks') for lv in FC.levels(tr) if len(lv[0]) > BT and chunks_with_splits(lv)[:2] == [0, 1]]
    assert hits
    assert sorted(FC.widest(tr)[0] for tr in trees_of('two_chunks')) == [304, 342]
    assert sorted(int(lv[1][-1]) for lv in hits) == [263, 285]


def test_four_chunks_a_level_of_more_than_768_nodes_splits_in_three_chunks_at_least():
    hits = [lv for tr in trees_of('four_chunks') for lv in FC.levels(tr) if len(lv[0]) > 3 * BT and len(chunks_with_splits(lv)) >= 3]
    assert hits
    assert any(chunks_with_splits(lv) == [0, 1, 2, 3] for lv in hits)
    assert FC.case('four_chunks')['prm']['max_depth'] == 12


def test_chunk_edge_a_level_of_exactly_256_nodes_then_a_wider_one():
    """The level of 256 fills its one chunk to the last lane (a split node at position 255); the level below has 257 nodes or more
    and splits in its second chunk."""
    ok = False
    for tr in trees_of('chunk_edge'):
        lv = FC.levels(tr)
        for k in range(len(lv) - 1):
            ok |= len(lv[k][0]) == BT and BT - 1 in lv[k][1] and len(lv[k + 1][0]) > BT and chunks_with_splits(lv[k + 1]) == [0, 1]
    assert ok


@pytest.mark.parametrize('n,n_tr', FC.SCAN_TILES)
def test_scan_tiles_sizes_and_a_split_in_every_tree(n, n_tr):
    c = FC.case('scan_tiles_%d_%d' % (n, n_tr))
    tr = c['jobs'][0][0]
    assert len(c['X']) == n and len(tr) == n_tr == len(np.unique(tr)) and not c['prm']['bootstrap']          # n_s == n_tr
    assert all(FC.n_splits(t) >= 1 for t in trees_of(c['name'])) and len(trees_of(c['name'])) == 3
    if (n, n_tr) == (1024, 257):            # packed into the first tiles of feature 0's list, scattered over the tiles of the others
        rank = [np.argsort(np.argsort(c['X'][:, f].astype(np.float32), kind='stable'), kind='stable')[tr] for f in (0, 1)]
        assert rank[0].max() == 256 and len(set(rank[1] // BT)) == 4
    if (n, n_tr) == (513, 256):
        assert (np.diff(tr) == 2).all()


def test_batches_case_is_two_jobs_of_seven_trees_on_the_two_chunk_rows():
    c, w = FC.case(FC.WORKER_CASE), FC.case('two_chunks')
    assert (c['X'] == w['X']).all() and (c['y'] == w['y']).all() and len(c['X']) == 4000
    assert len(c['jobs']) == 2 and c['prm']['n_trees'] == 7 and len(c['jobs'][1][1]) == 1000
    assert FC.WORKER_CASE not in FC.NAMES


def test_ties_twin_features_the_first_visited_one_is_chosen():
    c = FC.case('ties_twins')
    assert (c['X'][:, 3] == c['X'][:, 0]).all() and (c['X'][:, 4] == -c['X'][:, 1]).all()
    n = first_is_3 = 0
    for tree, trace in FC.traced('ties_twins'):
        for node, visited in trace:
            if 0 in visited and 3 in visited and tree['feature'][node] in (0, 3):
                first = 0 if visited.index(0) < visited.index(3) else 3
                assert tree['feature'][node] == first
                n += 1
                first_is_3 += first == 3
    assert n >= 10 and first_is_3 >= 1
    for (tree, _), want in zip(FC.traced('ties_twins'), trees_of('ties_twins')):        # (the traced run is the oracle's run)
        assert all((tree[f] == want[f]).all() for f in FC.FIELDS)


@pytest.mark.parametrize('name,n', [('ties_positions_8', 8), ('ties_positions_512', 512)])
def test_ties_two_positions_of_one_score_the_lower_one_is_chosen(name, n):
    c = FC.case(name)
    assert c['X'].shape == (n, 1) and c['prm']['max_features'] == 1 and not c['prm']['bootstrap']
    from tests import forest_fit_oracle as fo
    G = fo.g_table(n)
    r = n // 8
    score = lambda a0, a1: ((G[a0] + G[a1]) - G[a0 + a1]) + ((G[4 * r - a0] + G[4 * r - a1]) - G[8 * r - a0 - a1])         # noqa: E731
    tied = score(r, 0), score(3 * r, 4 * r)             # left of the cut: value 0 alone; everything but value 7
    others = [score(*np.bincount(c['y'][:p * r], minlength=2)) for p in range(2, 7)]
    assert tied[0] == tied[1] and tied[0] > max(others)
    assert (7 * r) // BT > r // BT or n == 8            # at 512 rows the two positions lie in different tiles of the list
    for tree in trees_of(name):
        assert tree['feature'][0] == 0 and tree['threshold'][0] == 0.5 and tree['n_node_samples'][tree['left'][0]] == r


def test_tiny_spreads_constant_by_the_1e_7_rule_and_a_node_nothing_can_split():
    c = FC.case('tiny_spreads')
    x32 = c['X'][:FC.TINY_N].astype(np.float32)
    one = np.float32(1.0)
    assert sorted(set(x32[:, 2])) == [np.nextafter(one, np.float32(0)), one] and sorted(set(x32[:, 3])) == [one, np.nextafter(one, np.float32(2))]
    thr = float(np.float32(1e-7))
    assert 0 < float(x32[:, 2].max()) - float(x32[:, 2].min()) <= thr < float(x32[:, 3].max()) - float(x32[:, 3].min())
    assert 0 < float(x32[:, 5].max()) - float(x32[:, 5].min()) <= thr and np.abs(x32[:, 6]).max() > 1e29
    feats = np.concatenate([t['feature'] for t in trees_of('tiny_spreads', 0)])
    used = np.bincount(feats[feats >= 0], minlength=7)
    assert used[2] == 0 and used[5] == 0 and used[3] > 0 and used[6] > 0
    past = [v for _, trace in FC.traced('tiny_spreads') for _, v in trace if len(v) > c['prm']['max_features']]
    assert len(past) >= 5 and sum(set(v[:2]) == {2, 5} for v in past) >= 3       # (others: columns constant in that node only)
    pts = c['X'][FC.TINY_N:]
    assert len(np.unique(pts, axis=0)) == 3 and all(len(np.unique(c['y'][FC.TINY_N + 20 * i:FC.TINY_N + 20 * i + 20])) == 2 for i in range(3))
    for t in trees_of('tiny_spreads', 1):
        stuck = FC.stuck_nodes(t, c['prm'])
        assert len(stuck) >= 1 and (t['impurity'][stuck] > 0).all()


@pytest.mark.parametrize('name', sorted(FC.DEGENERATE))
def test_degenerate_jobs(name):
    c, want = FC.case(name), FC.oracle(name)
    X, y, jobs, prm = c['X'], c['y'], c['jobs'], c['prm']
    assert len(X) == 20000 and X.shape[1] in (1, 9)
    assert [len(tr) for tr, _ in jobs] == [40, 1, 2, 50]
    assert [len(va) for _, va in jobs] == ([0, 0, 0, 0] if name.endswith('no_validation') else [0, 1, 257, 257])
    assert len(np.unique(y[jobs[0][0]])) == 1 and sorted(y[jobs[2][0]]) == [0, 1]
    size = lambda j: [len(t['left']) for t in want[j]['trees']]                          # noqa: E731
    assert size(0) == [1, 1, 1] and size(1) == [1, 1, 1]                                   # one class, one row: the root is a leaf
    deepest = max(int(FC.depths(t).max()) for t in want[3]['trees'])
    if prm['max_depth'] == 1:
        assert size(3) == [3, 3, 3] and size(2) == [1, 1, 1] and prm['min_samples_leaf'] == 5         # (two rows < 2 * 5)
    else:
        assert sorted(size(2)) == [1, 3, 3] and 3 <= deepest <= 30 and prm['min_samples_leaf'] == 1 and prm['min_samples_split'] == 2
    assert prm['max_features'] in (1, X.shape[1])


def test_degenerate_table_has_every_parameter_the_issue_names():
    prms = [FC.case(n)['prm'] for n in FC.DEGENERATE]
    ds = [FC.case(n)['X'].shape[1] for n in FC.DEGENERATE]
    assert {p['max_depth'] for p in prms} == {1, 30} and set(ds) == {1, 9}
    assert {(p['max_features'], d) for p, d in zip(prms, ds)} >= {(1, 9), (9, 9), (1, 1)}
    assert {(p['min_samples_leaf'], p['min_samples_split']) for p in prms} == {(1, 2), (5, 3)}


def test_on_thresholds_validation_values_that_equal_a_threshold_on_their_way():
    c = FC.case('on_thresholds')
    trees = trees_of('on_thresholds')
    th = np.unique(np.concatenate([t['threshold'][t['left'] >= 0] for t in trees]))
    assert set(th) <= {1.0, 2.0, 3.0, 4.0, 5.0} and {1.0, 3.0, 5.0} <= set(th)
    va = c['jobs'][0][1]
    assert len(va) == 1000 and len(c['jobs'][0][0]) == 3000 and len(trees) == 3
    hit = np.zeros(len(va), dtype=bool)
    for t in trees:
        hit |= FC.rows_on_a_threshold(t, c['X'][va])
    assert hit.sum() >= 100
    assert 0 < FC.oracle('on_thresholds')[0]['val_correct'] < 1000
