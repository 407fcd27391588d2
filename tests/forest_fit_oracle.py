"""CPU restatement of the random-forest fit behind `--train -c RF` (TEST INFRASTRUCTURE: only tests/ and tools/ import this; the
product never does).  The HIP kernel (mcaller_amd/csrc/mc_forest_fit.hip, k5_forest_fit) follows it bit for bit.

The reference fits RandomForestClassifier(bootstrap=True, criterion='entropy', max_depth=10, max_features=4, min_samples_leaf=2,
min_samples_split=3, n_estimators=50) with random_state=None (train_model.py:39-45), so no run reproduces another.  The tree
builder is scikit-learn's (sklearn/tree/_splitter.pyx node_split_best, _criterion.pyx Entropy, _tree.pyx DepthFirstTreeBuilder,
ensemble/_forest.py bootstrap); what it leaves to chance -- the bootstrap draws and the order the features of a node are drawn in --
is ours, from counter-based keys, so that the GPU can be compared with this file tree by tree:

* inputs cast to float32, as scikit-learn does;
* tree t of a job with seed s: tk = splitmix64(s + (t+1) 0x9E3779B97F4A7C15); draw i (0 <= i < n_tr) is
  train[((splitmix64(tk + i 0xD1342543DE82EF95) >> 32) n_tr) >> 32]; a row's weight is its draw count;
* node with heap id h (root 1, children 2h, 2h+1): nk = splitmix64(tk + h 0x632BE59BD9B4E019); Fisher-Yates of the d features,
  j = ((splitmix64(nk + i) >> 32) (i+1)) >> 32 for i = d-1 .. 1; features visited in that order until max_features were visited
  and one of them was not constant, or all d were;
* candidate splits: boundaries p where (double)x[p] > (double)x[p-1] + (double)1e-7f in the node's sorted values, both sides
  holding min_samples_leaf samples; score ((G[a0] + G[a1]) - G[a]) + ((G[b0] + G[b1]) - G[b]) with G[m] = m ln m (the entropy
  proxy times ln 2: the same maximiser); the highest score wins, ties to the feature visited first, then the lower position;
* threshold t = x[p-1]/2 + x[p]/2 (x[p-1] if that is x[p] or infinite); x <= t goes left;
* nodes in depth-first pre-order, left before right, with scikit-learn's fields.
"""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
DRAW = 0xD1342543DE82EF95
NODE = 0x632BE59BD9B4E019
THR = float(np.float32(1e-7))            # scikit-learn's FEATURE_THRESHOLD, a float32, compared in double
LN2 = float(np.log(2.0))
REFERENCE = dict(n_trees=50, max_depth=10, max_features=4, min_samples_split=3, min_samples_leaf=2, bootstrap=True)


def splitmix64(x):
    x = (x + GOLD) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def splitmix64_np(x):
    """splitmix64 of a uint64 array (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        x = x + np.uint64(GOLD)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def g_table(n):
    """G[m] = m ln m for m = 0 .. n (G[0] = 0): what the host hands the kernel."""
    m = np.arange(n + 1, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        G = m * np.log(m)
    G[0] = 0.0
    return G


def tree_key(seed, t):
    return splitmix64((seed + (t + 1) * GOLD) & M64)


def bootstrap_weights(train, n, tk, bootstrap=True):
    """Draw counts of the n rows of X for the tree with key tk (rows outside `train` keep weight 0)."""
    train = np.asarray(train, dtype=np.int64)
    if not bootstrap:
        return np.bincount(train, minlength=n).astype(np.int64)
    n_tr = len(train)
    i = np.arange(n_tr, dtype=np.uint64)
    with np.errstate(over='ignore'):
        u = splitmix64_np(np.uint64(tk) + i * np.uint64(DRAW)) >> np.uint64(32)
    pos = (u * np.uint64(n_tr)) >> np.uint64(32)
    return np.bincount(train[pos.astype(np.int64)], minlength=n).astype(np.int64)


def feature_order(tk, h, d):
    nk = splitmix64((tk + h * NODE) & M64)
    perm = list(range(d))
    for i in range(d - 1, 0, -1):
        j = ((splitmix64((nk + i) & M64) >> 32) * (i + 1)) >> 32
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def best_split(X32, y, w, idx, perm, G, max_features, msl):
    """-> (feature, threshold, visited features) of the node's best split, feature -1 if there is none."""
    d = X32.shape[1]
    wn = w[idx]
    c1 = wn * (y[idx] == 1)
    W1 = int(c1.sum())
    W0 = int(wn.sum()) - W1
    ns = len(idx)
    best, bf, bt = -np.inf, -1, -2.0
    n_vis = n_const = 0
    visited = []
    for f in perm:
        n_vis += 1
        visited.append(f)
        xs = X32[idx, f].astype(np.float64)
        o = np.argsort(xs, kind='stable')
        xv = xs[o]
        if xv[-1] <= xv[0] + THR:
            n_const += 1
        else:
            a1 = np.cumsum(c1[o])[:-1]                    # left = sorted positions [0, p), p = 1 .. ns-1
            a = np.cumsum(wn[o])[:-1]
            a0 = a - a1
            b0, b1 = W0 - a0, W1 - a1
            b = b0 + b1
            p = np.arange(1, ns)
            ok = (xv[1:] > xv[:-1] + THR) & (p >= msl) & (ns - p >= msl)
            if ok.any():
                s = ((G[a0] + G[a1]) - G[a]) + ((G[b0] + G[b1]) - G[b])
                s = np.where(ok, s, -np.inf)
                k = int(np.argmax(s))
                if s[k] > best:
                    best, bf = s[k], f
                    t = xv[k] / 2.0 + xv[k + 1] / 2.0
                    if t == xv[k + 1] or np.isinf(t):
                        t = xv[k]
                    bt = float(t)
        if not (n_vis < d and (n_vis < max_features or n_vis <= n_const)):
            break
    return bf, bt, visited


def fit_tree(X32, y, w, G, tk, max_depth=10, max_features=4, min_samples_split=3, min_samples_leaf=2, trace=None):
    """One tree on the rows with w > 0 -> dict of scikit-learn's node arrays (pre-order).  trace: a list that gets
    (node, visited features) for every split node (tests)."""
    d = X32.shape[1]
    rec = dict(left=[], right=[], feature=[], threshold=[], value=[], impurity=[], n_node_samples=[], weighted_n_node_samples=[])

    def grow(idx, depth, h):
        me = len(rec['left'])
        wn = w[idx]
        w1 = int(wn[y[idx] == 1].sum())
        W = int(wn.sum())
        w0 = W - w1
        ns = len(idx)
        rec['left'].append(-1)
        rec['right'].append(-1)
        rec['feature'].append(-2)
        rec['threshold'].append(-2.0)
        rec['value'].append((w0 / W, w1 / W))
        rec['impurity'].append(((G[W] - G[w0]) - G[w1]) / (W * LN2))
        rec['n_node_samples'].append(ns)
        rec['weighted_n_node_samples'].append(float(W))
        if depth >= max_depth or ns < min_samples_split or ns < 2 * min_samples_leaf or w0 == 0 or w1 == 0:
            return me
        f, t, visited = best_split(X32, y, w, idx, feature_order(tk, h, d), G, max_features, min_samples_leaf)
        if f < 0:
            return me
        rec['feature'][me], rec['threshold'][me] = f, t
        if trace is not None:
            trace.append((me, visited))
        go_left = X32[idx, f].astype(np.float64) <= t
        rec['left'][me] = grow(idx[go_left], depth + 1, 2 * h)
        rec['right'][me] = grow(idx[~go_left], depth + 1, 2 * h + 1)
        return me

    grow(np.nonzero(w > 0)[0], 0, 1)
    out = {k: np.asarray(v) for k, v in rec.items()}
    for k in ('left', 'right', 'feature', 'n_node_samples'):
        out[k] = out[k].astype(np.int32)
    out['value'] = out['value'].astype(np.float64).reshape(-1, 2)
    return out


def check_params(d, max_features):
    if max_features > d:
        raise ValueError('max_features must be in (0, n_features]: %d > %d' % (max_features, d))


def fit_forest(X, y, train, seed, G=None, n_trees=50, max_depth=10, max_features=4, min_samples_split=3, min_samples_leaf=2,
               bootstrap=True):
    """One job: list of n_trees trees (dicts of node arrays)."""
    X32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    y = np.asarray(y, dtype=np.int64)
    check_params(X32.shape[1], max_features)
    G = g_table(max(len(train), 1)) if G is None else G
    trees = []
    for t in range(n_trees):
        tk = tree_key(seed, t)
        w = bootstrap_weights(train, len(y), tk, bootstrap)
        trees.append(fit_tree(X32, y, w, G, tk, max_depth, max_features, min_samples_split, min_samples_leaf))
    return trees


def predict_proba(trees, X):
    """-> (P0, P1) as k3_forest adds them: per tree v_c / ((-0.0 + v0) + v1), summed in tree order, over the number of trees."""
    x = np.asarray(X, dtype=np.float64).astype(np.float32).astype(np.float64)
    P0 = np.zeros(len(x))
    P1 = np.zeros(len(x))
    rows = np.arange(len(x))
    for tr in trees:
        node = np.zeros(len(x), dtype=np.int64)
        while True:
            inner = tr['left'][node] >= 0
            if not inner.any():
                break
            f = np.where(inner, tr['feature'][node], 0)
            go = x[rows, f] <= tr['threshold'][node]
            node = np.where(inner, np.where(go, tr['left'][node], tr['right'][node]), node)
        v0, v1 = tr['value'][node, 0], tr['value'][node, 1]
        norm = (-0.0 + v0) + v1
        norm = np.where(norm == 0.0, 1.0, norm)
        P0 = P0 + v0 / norm
        P1 = P1 + v1 / norm
    return P0 / len(trees), P1 / len(trees)


def val_correct(trees, X, y):
    P0, P1 = predict_proba(trees, X)
    return int(((P1 > P0).astype(np.int64) == np.asarray(y, dtype=np.int64)).sum())


def fit_jobs(X, y, jobs, seeds, **prm):
    """What Device.forest_fit returns, job by job: trees and val_correct."""
    G = g_table(max(max(len(tr) for tr, _ in jobs), 1))
    out = []
    for (tr, va), s in zip(jobs, seeds):
        trees = fit_forest(X, y, tr, s, G, **prm)
        vc = val_correct(trees, np.asarray(X)[va], np.asarray(y)[va]) if len(va) else 0
        out.append(dict(trees=trees, val_correct=vc, n_val=len(va)))
    return out
