"""Synthetic classifiers and edge probes for the RF / LR / NBC / SVM paths, built directly from numpy at any number of inputs
(1 .. MC_MAX_K + 1) -- no scikit-learn.  TEST INFRASTRUCTURE: tests/test_clf_shapes.py pins the references on them, and
tests/test_gpu_clf_shapes.py holds k3_forest, k3_simple and k3_svm to those references.

Forests: every feature's thresholds come from a small pool, so that probes drawn from the same pool meet them exactly -- at a
float32 value, one float32 ulp either side, and as doubles whose float32 rounding lands on a threshold or crosses it (the kernel
and scikit-learn compare (double)(float)x <= threshold)."""
import numpy as np

from mcaller_amd.model_io import ForestWeights, GaussianNBWeights, LogisticWeights, SVMWeights

NODE = np.dtype([('left_child', '<i8'), ('right_child', '<i8'), ('feature', '<i8'), ('threshold', '<f8')])
CLASSES = ['A', 'm6A']


def _f32_neighbours(b):
    """(next float32 below b, next above b) for float32-representable b, as doubles."""
    b32 = np.float32(b)
    return float(np.nextafter(b32, np.float32(-np.inf))), float(np.nextafter(b32, np.float32(np.inf)))


def threshold_pool(rng, n_in, n_base=4, scale=3.0):
    """Per feature: float32 bases b; thresholds b (float32-representable), b + 0.3 gap and b + 0.7 gap (not representable; gap:
    the float32 spacing above b).  -> (thresholds [n_in] lists, probe values [n_in] arrays)."""
    thr, vals = [], []
    for _ in range(n_in):
        t_f, v_f = [], []
        for b in np.float32(rng.uniform(-scale, scale, size=n_base)):
            lo, hi = _f32_neighbours(b)
            b = float(b)
            gap = hi - b
            t_f += [b, b + 0.3 * gap, b + 0.7 * gap]
            v_f += [b, lo, hi,                               # on the threshold b, one float32 ulp either side
                    b + 0.1 * gap, b - 0.1 * (b - lo),       # doubles that round onto b
                    b + 0.4 * gap,                           # above b + 0.3 gap, rounds to b: at or below it as float32
                    b + 0.6 * gap]                           # below b + 0.7 gap, rounds to hi: above it as float32
        thr.append(t_f)
        vals.append(np.array(v_f))
    return thr, vals


def random_tree(rng, n_in, depth, thr, zero_leaf=0.0, leaf_values=None):
    """One tree of the given depth (0: a single leaf): one root-to-leaf path reaches the full depth, the other children stop
    early at random.  Leaf values: random class weights, (0, 0) with probability zero_leaf (the norm == 0 branch), or drawn
    from leaf_values (pairs)."""
    nodes, values = [], []

    def leaf():
        if rng.random() < zero_leaf:
            return (0.0, 0.0)
        if leaf_values is not None:
            return leaf_values[rng.integers(len(leaf_values))]
        return tuple(rng.uniform(0.0, 1.0, size=2))

    def build(d, spine):
        i = len(nodes)
        nodes.append(None)
        values.append(None)
        if d == 0 or (not spine and rng.random() < 0.4):
            nodes[i] = (-1, -1, -2, -2.0)
            values[i] = leaf()
            return i
        f = int(rng.integers(n_in))
        t = thr[f][rng.integers(len(thr[f]))]
        go_left = rng.random() < 0.5
        left = build(d - 1, spine and go_left)
        right = build(d - 1, spine and not go_left)
        nodes[i] = (left, right, f, t)
        values[i] = tuple(rng.uniform(0.0, 1.0, size=2))    # (internal nodes' values are never read)
        return i

    build(depth, True)
    return np.array(nodes, dtype=NODE), np.array(values, dtype=np.float64).reshape(len(nodes), 1, 2)


def forests(rng, n_in, n_trees, depth=(0, 12), thr=None, zero_leaf=0.05, single_leaf=0.05, leaf_values=None):
    """ForestWeights per entry of n_trees (trees per sub-model, ragged), depths drawn from the range."""
    if thr is None:
        thr, _ = threshold_pool(rng, n_in)
    out = []
    for nt in n_trees:
        trees = []
        for _ in range(nt):
            d = 0 if rng.random() < single_leaf else int(rng.integers(depth[0], depth[1] + 1))
            trees.append(random_tree(rng, n_in, d, thr, zero_leaf, leaf_values))
        out.append(ForestWeights(trees, n_in, CLASSES))
    return out


def forest_probes(rng, vals, n):
    """n rows, every feature drawn from its pool of edge values (vals from threshold_pool)."""
    return np.stack([v[rng.integers(len(v), size=n)] for v in vals], axis=1)


def forest_case(seed, n_in, n_trees, depth=(0, 12)):
    """A ragged forest set and its edge probes (1000 rows per sub-model and one past them)."""
    rng = np.random.default_rng(seed)
    thr, vals = threshold_pool(rng, n_in)
    f = forests(rng, n_in, n_trees, depth, thr)
    X = forest_probes(rng, vals, 1000 * (len(f) + 1))
    sub = np.repeat(np.arange(len(f) + 1), 1000).astype(np.uint8)
    rng.shuffle(sub)
    return f, X, sub


def logistic_models(rng, n_in, n_models=2):
    return [LogisticWeights(rng.normal(0, 1.0, n_in), rng.normal(0, 0.5), CLASSES) for _ in range(n_models)]


def logistic_probes(rng, w, n_random=200):
    """Rows whose decision value is moderate, past where exp over/underflows (|d| ~ 709 / 745) and far out
    (p exactly 0 or 1), and random rows."""
    n_in = w.n_in
    targets = np.array([0.5, -0.5, 3.0, -3.0, 20.0, -20.0, 40.0, -40.0, 700.0, -700.0, 709.5, -709.5, 720.0, -720.0,
                        744.0, -744.0, 746.0, -746.0, 800.0, -800.0, 1e4, -1e4])
    i = int(np.argmax(np.abs(w.coef)))
    X = rng.normal(0, 1.0, size=(len(targets), n_in))
    X[:, i] = 0.0
    X[:, i] = (targets - (X @ w.coef + w.intercept)) / w.coef[i]
    return np.concatenate([X, rng.normal(0, 3.0, size=(n_random, n_in))])


def logistic_exact_half(n_in):
    """A model and a row whose decision value is 0.0 exactly whatever the order of the sum: coefficients and inputs powers of two."""
    coef = np.array([0.5 * (-1) ** j * 2.0 ** -(j % 3) for j in range(n_in)])
    w = LogisticWeights(coef, 0.0 if n_in % 2 == 0 else coef[-1] * -2.0, CLASSES)
    x = np.zeros((1, n_in))
    if n_in % 2 == 0:
        x[0, :] = [2.0 ** (j % 3) for j in range(n_in)]          # +1, -1, +1, ... in pairs
    else:
        x[0, -1] = 2.0                                       # coef[-1] * 2 + intercept == 0
    return w, x


def gnb_models(rng, n_in, n_models=2):
    out = []
    for _ in range(n_models):
        theta = rng.normal(0, 2.0, size=(2, n_in))
        var = rng.uniform(0.2, 3.0, size=(2, n_in))
        prior = rng.dirichlet([5.0, 5.0])
        out.append(GaussianNBWeights(theta, var, prior, CLASSES))
    return out


def gnb_tiny_var(rng, n_in):
    """Variances of 1e-9 .. 1e-6: the joint log likelihoods of any row off the means differ by 1e6 and more (p exactly 0 / 1)."""
    theta = rng.normal(0, 1.0, size=(2, n_in))
    var = 10.0 ** rng.uniform(-9, -6, size=(2, n_in))
    return GaussianNBWeights(theta, var, np.array([0.3, 0.7]), CLASSES)


def gnb_tie(rng, n_in, var=None):
    """Equal variances and priors, the class means mirrored around a row -> that row's two jll are equal bit for bit.  var: one
    variance for every input (small: |jll| in the millions at that row and near it)."""
    x = np.round(rng.normal(0, 1.0, n_in) * 8.0) / 8.0           # (eighths: x -+ delta are exact)
    delta = 2.0 ** rng.integers(-3, 3, size=n_in).astype(np.float64)
    theta = np.stack([x - delta, x + delta])
    v = rng.uniform(0.5, 2.0, n_in) if var is None else np.full(n_in, float(var))
    return GaussianNBWeights(theta, np.tile(v, (2, 1)), np.array([0.5, 0.5]), CLASSES), x[None, :]


def gnb_near_tie_probes(rng, w, x, n=40):
    """Rows next to the tie row x of a gnb_tie model: the jll differ by O(1) (p anywhere in (0, 1)) however large they are -- where
    the order of the sums over the inputs shows in p."""
    d = np.abs(w.theta[1] - w.theta[0])
    return x + rng.normal(0, 1.0, size=(n, w.n_in)) * 0.5 * w.var[0] / (d * np.sqrt(w.n_in))


def gnb_probes(rng, w, n_random=200):
    """Random rows near the class means, far out (|x| up to 1e4: huge jll differences), and rows between the means."""
    near = w.theta[rng.integers(2, size=n_random)] + rng.normal(0, 1.5, size=(n_random, w.n_in))
    far = rng.normal(0, 1.0, size=(60, w.n_in)) * 10.0 ** rng.uniform(1, 4, size=(60, 1))
    t = rng.uniform(0, 1, size=(60, 1))
    mid = w.theta[0] * t + w.theta[1] * (1 - t)
    return np.concatenate([near, far, mid])


def svm_model(rng, n_in, n_sv, gamma=None, A=None, B=0.05, intercept=None):
    sv = rng.normal(0, 2.0, size=(n_sv, n_in))
    coef = rng.uniform(-1, 1, size=n_sv)
    g = 0.5 / n_in if gamma is None else gamma
    return SVMWeights(sv, coef, g, rng.normal(0, 0.3) if intercept is None else intercept, -1.0 if A is None else A, B, CLASSES)


def svm_scaled(rng, n_in, n_sv, gamma=None):
    """An SVM whose Platt A maps the decision values of rows near the support vectors to f = dec A + B in about [-60, 60]: past
    the 1e-7 clamp on both sides."""
    from tests import svm_oracle
    w = svm_model(rng, n_in, n_sv, gamma)
    X = rng.normal(0, 2.0, size=(256, n_in))
    d = svm_oracle.decision(w.sv, w.dual_coef, w.gamma, w.intercept, X)
    span = max(np.abs(d - np.median(d)).max(), 1e-6)
    return SVMWeights(w.sv, w.dual_coef, w.gamma, w.intercept - np.median(d), -60.0 / span, 0.0, CLASSES)


# f = dec A + B: in the band (|f| < ln(0.505 / 0.495) = 0.0200007: p = 1/2 exactly), just outside it, either side of the clamp at
# s = 1e-7 (|f| = 16.118), far past it
SVM_F_TARGETS = (0.0, 0.005, -0.005, 0.0199, -0.0199, 0.02002, -0.02002, 0.05, -0.05, 16.0, -16.0, 16.3, -16.3, 25.0, -25.0)


def svm_band_probes(rng, w, targets=SVM_F_TARGETS):
    """Rows whose f = dec A + B is each target: bisection on f along a segment between a row with f below and one above, all
    targets at once (the decision value summed by numpy here: the targets are 1e-6 and more from the edges they straddle).  The
    targets the segment does not span are skipped."""
    def f_of(X):
        d2 = ((X[:, None, :] - w.sv[None, :, :]) ** 2).sum(axis=2)
        return (np.exp(-w.gamma * d2) @ w.dual_coef + w.intercept) * w.A + w.B
    cand = rng.normal(0, 2.0, size=(256, w.n_in))
    f = f_of(cand)
    t = np.array([x for x in targets if f.min() < x < f.max()])
    lo, hi = cand[int(np.argmin(f))], cand[int(np.argmax(f))]
    a, b = np.tile(lo, (len(t), 1)), np.tile(hi, (len(t), 1))
    for _ in range(64):
        m = 0.5 * (a + b)
        below = (f_of(m) < t)[:, None]
        a, b = np.where(below, m, a), np.where(below, b, m)
    return (0.5 * (a + b)).reshape(-1, w.n_in)


def assert_matches(got, want, tol):
    """|got - want| <= tol and the same labels (p >= 0.5), NaN in the same places; where want is exactly 0, 1/2 or 1, got is too."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'scored / unscored rows differ'
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
    assert err <= tol, 'probability differs by %g' % err
    assert np.array_equal(got[ok] >= 0.5, want[ok] >= 0.5), 'a label differs'
    for v in (0.0, 0.5, 1.0):
        at = ok & (want == v)
        assert np.all(got[at] == v), (v, got[at][got[at] != v][:4])
    return err
