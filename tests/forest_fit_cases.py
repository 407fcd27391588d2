"""Problems for the random-forest fit kernel (k5_forest_fit, k5_forest_val: csrc/mc_forest_fit.hip), one per path the kernel takes,
and small helpers on the trees of tests/forest_fit_oracle.py.  The yardstick of every case is fo.fit_jobs on the same rows, jobs,
seeds and parameters (`oracle(name)`, computed once per process and shared); tests/test_forest_fit_cases.py proves without a GPU,
from the oracle's trees alone, that every case reaches the path it names, tests/test_gpu_forest_fit_edges.py holds the device
against the oracle byte for byte.

What the kernel does with a case (read from mc_forest_fit.hip, restated here so that the CPU file can check the table):
  * a tree is one workgroup of BT = 256 threads; the open nodes of a level are walked in chunks of BT, and from the second chunk on
    the ranks of the split nodes and the counts of their left rows continue from the chunks before;
  * the n rows of X (compaction) and the n_s in-bag rows (stable partition) are walked in tiles of BT;
  * trees are grown `batch` at a time (MCALLER_FOREST_MEM_MB, read once per process: tests/_forest_fit_worker.py);
  * k5_forest_val's grid is sized by the job with the most validation rows and is not launched when no job has any."""
import functools

import numpy as np

from tests import forest_fit_oracle as fo
from tests.test_gpu_forest_fit import FIELDS, assert_same_forest, data          # (its comparison and its data, as they are)

BT = 256                   # threads of a workgroup: the chunk of a level and the tile of the two block scans


# ---- data ----
def continuous(n, d, seed):
    """The suite's continuous data: normal columns of growing spread, a last column of four values, noisy labels."""
    return data(n, d, seed)


def grid(n, d=7, seed=3, hi=4, scale=2.0):
    """Four values per feature and a parity label: nothing splits cleanly, so the trees stay wide down to max_depth."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, hi, (n, d)) * scale
    y = ((X.sum(1) // 2) % 2).astype(np.uint8)
    return X, y


def _case(name, X, y, jobs, seeds, **prm):
    p = dict(fo.REFERENCE)
    p.update(prm)
    none = np.zeros(0, np.int64)
    jobs = [(np.asarray(tr, dtype=np.int64), none if va is None else np.asarray(va, dtype=np.int64)) for tr, va in jobs]
    assert len(jobs) == len(seeds)
    return dict(name=name, X=np.ascontiguousarray(X, dtype=np.float64), y=np.ascontiguousarray(y, dtype=np.uint8), jobs=jobs,
                seeds=list(seeds), prm=p)


# ---- the cases ----
# (3) a level of exactly BT nodes: search_chunk_edge()'s first hit (a CPU search over sizes and data seeds of `grid`, the oracle
# alone); max_depth = 11 lets the 288 nodes below that level split once more, in two chunks
EDGE_ROWS, EDGE_DATA_SEED, EDGE_SEED, EDGE_TREES = 3500, 5, 77, 2
SCAN_TILES = ((255, 255), (256, 256), (257, 257), (512, 512), (513, 513), (513, 256), (1024, 257))


def _wide(n, **prm):
    X, y = grid(n)
    return X, y, [(np.arange(n), None)], [77], dict(dict(n_trees=2), **prm)


def _scan_tile(n, n_tr):
    X, y = continuous(n, 7, 1000 * n + n_tr)
    rows = np.arange(n)
    if n_tr == n:
        tr = rows
    elif (n, n_tr) == (513, 256):
        tr = rows[1::2]                                      # every other row of 513
    else:
        tr = np.sort(np.argsort(X[:, 0].astype(np.float32), kind='stable')[:n_tr])     # the first rows of feature 0's sorted list
    assert len(tr) == n_tr
    return X, y, [(tr, np.setdiff1d(rows, tr))], [77], dict(n_trees=3, bootstrap=False)


def _batches():
    X, y = grid(4000)
    rows = np.arange(4000)
    return X, y, [(rows, None), (rows[rows % 4 != 0], rows[rows % 4 == 0])], [77, 78], dict(n_trees=7)


def _ties_twins():
    X, y = continuous(600, 6, 9)
    X[:, 3] = X[:, 0]
    X[:, 4] = -X[:, 1]
    rows = np.arange(600)
    return X, y, [(rows[rows % 4 != 0], rows[rows % 4 == 0])], [77], dict(n_trees=6)


def _ties_positions(reps):
    """One feature, values 0..7 (`reps` rows each), labels 0 1 1 0 0 1 1 0: cutting after the first value and before the last one
    leave mirrored halves, the two scores are the same sum with its two terms swapped, and the lower position has to win."""
    x = np.repeat(np.arange(8.0), reps)
    y = np.repeat(np.array([0, 1, 1, 0, 0, 1, 1, 0], dtype=np.uint8), reps)
    rows = np.arange(len(x))
    return x[:, None], y, [(rows, rows)], [77], dict(n_trees=2, bootstrap=False, max_features=1, min_samples_leaf=1, min_samples_split=2)


TINY_N = 600               # rows of the 1e-7 case's first job; its second job: 3 points x 20 rows behind them


def _tiny_spreads():
    """Feature 2: 1.0 - k * 2e-8, k in 0..4.  In float32 (spacing 2^-24 below 1) two values remain, 1.0 (k = 0, 1) and 1 - 2^-24
    (k = 2, 3, 4): a spread of 5.96e-8, positive and at most 1e-7f, so the column counts as constant in every node and the node
    visits one feature more (the +64 path).  Feature 3: 1.0 + k * 2e-8: above 1 the spacing is 2^-23, what remains is 1.0
    (k = 0, 1, 2) and 1 + 2^-23 (k = 3, 4), 1.19e-7 apart: just MORE than 1e-7f, so this column is no constant and a boundary between
    its two values is a candidate.  Feature 5: data * 1e-30 (whole spread below 1e-7: never a split feature), feature 6: data * 1e30.
    The second job: 3 distinct points, 20 rows each, labels mixed within a point: once a node holds one point, every feature is
    constant, and the node stays without a split though it is no leaf by the rules.  max_features = 2: a node goes on past
    max_features only while everything it visited was constant, and with two such columns (2 and 5) that happens once in 21 nodes."""
    X, y = continuous(TINY_N, 7, 11)
    rng = np.random.default_rng(12)
    X[:, 2] = 1.0 - rng.integers(0, 5, TINY_N) * 2e-8
    X[:, 3] = 1.0 + rng.integers(0, 5, TINY_N) * 2e-8
    X[:, 6] = X[:, 5] * 1e30
    X[:, 5] = X[:, 5] * 1e-30
    P = continuous(3, 7, 13)[0]
    X = np.concatenate([X, np.repeat(P, 20, axis=0)])
    y = np.concatenate([y, (np.arange(60) % 3 == 0).astype(np.uint8)])
    rows = np.arange(TINY_N)
    pts = np.arange(TINY_N, TINY_N + 60)
    return X, y, [(rows[rows % 4 != 0], rows[rows % 4 == 0]), (pts, pts)], [77, 78], dict(n_trees=6, max_features=2)


DEGENERATE_N = 20000


def _degenerate(d, no_val=False, **prm):
    """Jobs that hardly are any, in one call: training rows of one class (the root is a leaf), one training row, two, 50 of 20 000;
    validation sets of 0, 1, 257 and 257 rows (k5_forest_val's grid is sized by the largest; none at all with no_val)."""
    rng = np.random.default_rng(21 + d)
    if d > 1:
        X, y = continuous(DEGENERATE_N, d, 20 + d)
    else:
        X = np.round(rng.normal(size=(DEGENERATE_N, 1)), 1)
        y = (rng.random(DEGENERATE_N) < 1.0 / (1.0 + np.exp(-2.0 * X[:, 0]))).astype(np.uint8)
    rows = np.arange(DEGENERATE_N)
    one_class = rows[y == 0][:40]
    two = np.array([rows[y == 0][50], rows[y == 1][50]])
    fifty = rows[199::400]
    assert len(fifty) == 50 and len(np.unique(y[fifty])) == 2
    jobs = [(one_class, None), (rows[7:8], rows[9:10]), (two, rows[1000:1257]), (fifty, rows[3000:3257])]
    if no_val:
        jobs = [(tr, None) for tr, _ in jobs]
    return X, y, jobs, [77, 78, 81, 80], dict(dict(n_trees=3), **prm)        # (seed 81: the two rows are drawn both, and one twice)


SMALL = dict(min_samples_leaf=1, min_samples_split=2)
DEGENERATE = {
    'degenerate_d9_depth30_all_features': lambda: _degenerate(9, max_depth=30, max_features=9, **SMALL),
    'degenerate_d9_depth1_one_feature': lambda: _degenerate(9, max_depth=1, max_features=1, min_samples_leaf=5),
    'degenerate_d1_depth30': lambda: _degenerate(1, max_depth=30, max_features=1, **SMALL),
    'degenerate_d1_depth1_leaf5': lambda: _degenerate(1, max_depth=1, max_features=1, min_samples_leaf=5),
    'degenerate_no_validation': lambda: _degenerate(9, no_val=True, max_depth=30, max_features=9, **SMALL),
}

ON_THRESHOLD_TRAIN, ON_THRESHOLD_VAL = 3000, 1000


def _on_thresholds():
    """Training values 0, 2, 4, 6: every threshold is a whole number 1 .. 5.  Validation values 0 .. 6: many sit on a threshold."""
    X, y = grid(ON_THRESHOLD_TRAIN)
    Xv, yv = grid(ON_THRESHOLD_VAL, seed=4, hi=7, scale=1.0)
    rows = np.arange(ON_THRESHOLD_TRAIN + ON_THRESHOLD_VAL)
    return np.concatenate([X, Xv]), np.concatenate([y, yv]), [(rows[:ON_THRESHOLD_TRAIN], rows[ON_THRESHOLD_TRAIN:])], [77], dict(n_trees=3)


def _edge():
    X, y = grid(EDGE_ROWS, seed=EDGE_DATA_SEED)
    return X, y, [(np.arange(EDGE_ROWS), None)], [EDGE_SEED], dict(n_trees=EDGE_TREES, max_depth=11)


def search_chunk_edge(sizes=range(3000, 4001, 100), data_seeds=range(3, 13)):
    """How EDGE_ROWS and EDGE_DATA_SEED were found (17 s on one core; no test runs it): the first (rows, data seed) of `grid` at
    which a tree of the reference parameters has a level of exactly BT nodes and a wider one."""
    for n in sizes:
        for ds in data_seeds:
            X, y = grid(n, seed=ds)
            for tr in fo.fit_forest(X, y, np.arange(n), EDGE_SEED, **dict(fo.REFERENCE, n_trees=EDGE_TREES)):
                w = [len(nodes) for nodes, _ in levels(tr)]
                if BT in w and max(w) > BT:
                    return n, ds
    return None


MAKERS = {
    'two_chunks': lambda: _wide(4000),
    'four_chunks': lambda: _wide(12000, max_depth=12),
    'chunk_edge': _edge,
    'batches': _batches,
    'ties_twins': _ties_twins,
    'ties_positions_8': lambda: _ties_positions(1),
    'ties_positions_512': lambda: _ties_positions(64),
    'tiny_spreads': _tiny_spreads,
    'on_thresholds': _on_thresholds,
}
MAKERS.update({'scan_tiles_%d_%d' % s: functools.partial(_scan_tile, *s) for s in SCAN_TILES})
MAKERS.update(DEGENERATE)
WORKER_CASE = 'batches'
# every case but the one the worker runs in processes of its own
NAMES = [k for k in MAKERS if k != WORKER_CASE]


@functools.lru_cache(maxsize=None)
def case(name):
    X, y, jobs, seeds, prm = MAKERS[name]()
    return _case(name, X, y, jobs, seeds, **prm)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """fo.fit_jobs of the case: per job its trees and val_correct.  Computed once, shared, never changed."""
    c = case(name)
    return fo.fit_jobs(c['X'], c['y'], c['jobs'], c['seeds'], **c['prm'])


def device_fit(dev, name):
    c = case(name)
    return dev.forest_fit(c['X'], c['y'], c['jobs'], seeds=c['seeds'], **c['prm'])


def traced(name, job=0):
    """The case's job once more with fit_tree's trace: per tree (tree, [(node, visited features)] of its split nodes)."""
    c = case(name)
    p = c['prm']
    X32 = c['X'].astype(np.float32)
    y = c['y'].astype(np.int64)
    train = c['jobs'][job][0]
    G = fo.g_table(max(len(tr) for tr, _ in c['jobs']))
    out = []
    for t in range(p['n_trees']):
        tk = fo.tree_key(c['seeds'][job], t)
        w = fo.bootstrap_weights(train, len(y), tk, p['bootstrap'])
        trace = []
        out.append((fo.fit_tree(X32, y, w, G, tk, p['max_depth'], p['max_features'], p['min_samples_split'], p['min_samples_leaf'], trace), trace))
    return out


# ---- helpers on the oracle's trees ----
def depths(tree):
    """Depth of every node of a pre-order tree."""
    dep = np.zeros(len(tree['left']), dtype=np.int64)
    for v in range(len(dep)):
        if tree['left'][v] >= 0:
            dep[tree['left'][v]] = dep[tree['right'][v]] = dep[v] + 1
    return dep


def levels(tree):
    """Per depth (nodes, split_positions): the nodes of that depth in pre-order -- which is the kernel's level order: the children
    of the split nodes, left before right, in the order of their parents -- and the positions among them of those that split."""
    dep = depths(tree)
    out = []
    for k in range(int(dep.max()) + 1):
        nodes = np.nonzero(dep == k)[0]
        out.append((nodes, np.nonzero(tree['left'][nodes] >= 0)[0]))
    return out


def widest(tree):
    """(nodes, last split position) of the tree's widest level."""
    nodes, pos = max(levels(tree), key=lambda lv: len(lv[0]))
    return len(nodes), (int(pos[-1]) if len(pos) else -1)


def n_splits(tree):
    return int((tree['left'] >= 0).sum())


def rows_on_a_threshold(tree, X):
    """Per row of X: whether a node on the row's way down compares a value that EQUALS the node's threshold (`<=` goes left)."""
    x = np.asarray(X, dtype=np.float64).astype(np.float32).astype(np.float64)
    hit = np.zeros(len(x), dtype=bool)
    for i in range(len(x)):
        v = 0
        while tree['left'][v] >= 0:
            xv, th = x[i, tree['feature'][v]], tree['threshold'][v]
            hit[i] |= xv == th
            v = tree['left'][v] if xv <= th else tree['right'][v]
    return hit


def stuck_nodes(tree, prm):
    """Nodes that no rule makes a leaf (depth, sizes, both classes present) and that still have no split."""
    dep = depths(tree)
    ns = tree['n_node_samples']
    mixed = (tree['value'][:, 0] > 0) & (tree['value'][:, 1] > 0)
    open_ = (dep < prm['max_depth']) & (ns >= prm['min_samples_split']) & (ns >= 2 * prm['min_samples_leaf']) & mixed
    return np.nonzero(open_ & (tree['left'] < 0) & (tree['feature'] == -2))[0]


def assert_same_jobs(got, want, jobs):
    assert len(got) == len(want) == len(jobs)
    for j, (g, w) in enumerate(zip(got, want)):
        assert_same_forest(g, w['trees'])
        assert g['val_correct'] == w['val_correct'] and g['n_val'] == len(jobs[j][1]), 'job %d' % j
