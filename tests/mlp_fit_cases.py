"""Small problems for the MLP fit kernel (k4_mlp_fit, csrc/mc_train.hip), one per edge of the kernel: a seeded generator and a named
table.  A case is the smallest problem that still reaches the edge it names.  The yardstick is oracle/mlp_fit_oracle.py::fit on the
same rows, seeds and parameters (`oracle(case)`, computed once per process); tests/test_mlp_fit_cases.py checks on the CPU that
every case reaches its edge and keeps the margins the device tests rely on, tests/test_gpu_mlp_fit_shapes.py holds the kernel
against it.

What the kernel does with a case (read from mc_train.hip, restated here so that the CPU file can check the table):
  * batch_size >= 64 -> four workgroups per fit (GW = 16 waves), below -> one (GW = 4); wave gw takes rows gw and gw + GW of a
    batch together and pads a missing second row with the first;
  * lane l owns hidden units l and l + 64; the loops over inputs are unrolled over 9 and masked by the input count;
  * the epoch's order is a Feistel permutation on the next EVEN power of two >= n, cycle-walked into range;
  * up to eight fits are numbered by XCD, more are numbered plainly."""
import functools

import numpy as np

from oracle import mlp_fit_oracle as mo

N_VAL = 40                 # held-out rows of a job that trains on all rows (appended after the training rows)
WAVES = 4                  # waves per workgroup (MC_FIT_WAVES)


def workgroups(batch_size):
    """Workgroups per fit as mc_mlp_fit picks them (without MCALLER_FIT_WGS, and while the device holds them all)."""
    return 4 if batch_size >= 64 else 1


def perm_bits(n):
    """Width of the Feistel network for n rows (mo.feistel_perm and the kernel)."""
    bits = max(2, (n - 1).bit_length())
    return bits + (bits & 1)


def _case(name, edge, n, d, hidden, batch_size, max_iter=8, seeds=(5,), jobs='all', data_seed=1, **other):
    """jobs: 'all' -- one job per seed, each on all n rows, N_VAL further rows held out;
             ('folds', k) -- k jobs, job f trains on the rows i % k != f and holds out the others;
             ('folds+whole', k) -- the k folds, then all n rows with N_VAL further rows held out;
             'empty_middle' -- three jobs on all n rows, the middle one WITHOUT training rows (held-out rows only).
    other: shuffle, tol, n_iter_no_change, x_scale, init ('aligned+8' / 'aligned-8'), expect (what the CPU file checks)."""
    c = dict(name=name, edge=edge, n=n, d=d, hidden=hidden, batch_size=batch_size, max_iter=max_iter, seeds=tuple(seeds), jobs=jobs,
             data_seed=data_seed, shuffle=True, tol=1e-4, n_iter_no_change=10, x_scale=1.0, init=None, expect={})
    assert set(other) <= set(c), other
    c.update(other)
    return c


# data seeds other than 1: picked so that no held-out row has the oracle's p within 1e-4 of 0.5 and, for the stopping cases, so that no
# epoch's loss comes within 1e-5 of best - tol (conditions on the inputs: tests/test_mlp_fit_cases.py holds both for every case)
DATA_SEEDS = {'last_batch_1_one_wg': 3, 'stop_batch_200': 3}


def _table():
    t = []
    # ---- hidden widths at the lane boundary (a lane owns units l and l + 64), on both paths ----
    for h in (1, 2, 63, 64, 65, 100, 127, 128):
        t.append(_case('width_%d_four_wgs' % h, 'width', 150, 7, h, 64, expect=dict(wgs=4)))
        t.append(_case('width_%d_one_wg' % h, 'width', 80, 7, h, 32, expect=dict(wgs=1)))
    # ---- input counts: the loops are unrolled over 9 and masked ----
    for d in (1, 2, 8, 9):
        t.append(_case('inputs_%d_four_wgs' % d, 'inputs', 150, d, 65, 64, expect=dict(wgs=4)))
        t.append(_case('inputs_%d_one_wg' % d, 'inputs', 80, d, 65, 32, expect=dict(wgs=1)))
    # ---- the last batch around GW and 2 GW rows (16 / 32 with four workgroups, 4 / 8 with one) ----
    for r in (1, 2, 15, 16, 17, 31, 32, 33, 63):
        t.append(_case('last_batch_%d_four_wgs' % r, 'last_batch', 64 + r, 7, 65, 64, expect=dict(wgs=4, last_batch=r, batches=2)))
    for r in (1, 3, 4, 5, 7, 8, 9, 15):
        t.append(_case('last_batch_%d_one_wg' % r, 'last_batch', 16 + r, 7, 65, 16, expect=dict(wgs=1, last_batch=r, batches=2)))
    for n in (1, 2, 3):
        t.append(_case('rows_%d_four_wgs' % n, 'short', n, 7, 65, 64, expect=dict(wgs=4, last_batch=n, batches=1)))
        t.append(_case('rows_%d_one_wg' % n, 'short', n, 7, 65, 32, expect=dict(wgs=1, last_batch=n, batches=1)))
    t.append(_case('rows_63_batch_200', 'short', 63, 7, 65, 200, expect=dict(wgs=4, last_batch=63, batches=1)))
    # ---- batch sizes: the switch between one and four workgroups; every thread stages a row ----
    t.append(_case('batch_63', 'batch', 200, 7, 65, 63, expect=dict(wgs=1, last_batch=11, batches=4)))
    t.append(_case('batch_64', 'batch', 200, 7, 65, 64, expect=dict(wgs=4, last_batch=8, batches=4)))
    t.append(_case('batch_255', 'batch', 600, 9, 128, 255, expect=dict(wgs=4, last_batch=90, batches=3)))
    t.append(_case('batch_256', 'batch', 600, 9, 128, 256, expect=dict(wgs=4, last_batch=88, batches=3)))
    # ---- the epoch permutation on either side of an even power of two: `half` and `mask` change, cycle-walking starts ----
    for n, bs, bits in ((16, 4, 4), (17, 4, 6), (64, 16, 6), (65, 16, 8), (256, 64, 8), (257, 64, 10), (1024, 200, 10), (1025, 200, 12)):
        t.append(_case('perm_%d' % n, 'perm', n, 7, 16, bs, seeds=(31, 77), expect=dict(bits=bits, walks=(1 << bits) > n, min_batches=3)))
    # ---- the stopping rule under shuffling; fits of one call that leave the epoch loop at different times ----
    t.append(_case('stop_batch_200', 'stop', 450, 7, 16, 200, max_iter=60, seeds=(41, 42, 43, 44, 45, 46), jobs=('folds+whole', 5),
                   tol=1e-2, n_iter_no_change=2, expect=dict(wgs=4)))
    t.append(_case('stop_batch_32', 'stop', 450, 7, 16, 32, max_iter=25, seeds=(51, 52, 53, 54, 55, 56), jobs=('folds+whole', 5),
                   tol=1e-2, n_iter_no_change=2, expect=dict(wgs=1)))
    # ---- clipped probabilities: |output| > 700, exp overflows, p is exactly 0 or 1 and the clip decides the loss ----
    for sign in ('+8', '-8'):
        t.append(_case('clip_%s_four_wgs' % sign, 'clip', 150, 7, 100, 64, init='aligned' + sign, x_scale=30.0, expect=dict(wgs=4)))
        t.append(_case('clip_%s_one_wg' % sign, 'clip', 80, 7, 100, 32, init='aligned' + sign, x_scale=30.0, expect=dict(wgs=1)))
    # ---- job counts: fits are numbered by XCD up to eight and plainly from nine; a job without training rows ----
    t.append(_case('jobs_8', 'jobs', 150, 7, 16, 64, seeds=range(61, 69), jobs=('folds', 8), expect=dict(wgs=4, fold_sizes=(18, 19))))
    t.append(_case('jobs_9', 'jobs', 150, 7, 16, 64, seeds=range(71, 80), jobs=('folds', 9), expect=dict(wgs=4, fold_sizes=(16, 17))))
    t.append(_case('empty_middle_four_wgs', 'empty', 100, 7, 65, 64, seeds=(81, 82, 83), jobs='empty_middle', expect=dict(wgs=4)))
    t.append(_case('empty_middle_one_wg', 'empty', 100, 7, 65, 32, seeds=(81, 82, 83), jobs='empty_middle', expect=dict(wgs=1)))
    for name, seed in DATA_SEEDS.items():
        [c] = [c for c in t if c['name'] == name]
        c['data_seed'] = seed
    return {c['name']: c for c in t}


CASES = _table()

# the product's shape, run under MCALLER_FIT_WGS = 1, 2 and 8 in processes of their own (tests/_mlp_fit_worker.py)
WORKER_CASE = _case('product_shape', 'groups', 450, 7, 100, 200, max_iter=12, seeds=(91, 92, 93, 94, 95, 96), jobs=('folds+whole', 5))


def problem(case):
    """-> X [n + N_VAL, d], y: rows of a noisy linear rule, both classes among the first n rows (where there are two rows)."""
    rng = np.random.default_rng([case['data_seed'], case['n'], case['d']])
    n_all = case['n'] + N_VAL
    X = rng.normal(size=(n_all, case['d']))
    w = direction(case)
    y = (X @ w + 0.8 * rng.normal(size=n_all) > 0).astype(np.uint8)
    if case['n'] >= 2 and len(np.unique(y[:case['n']])) < 2:
        y[0], y[1] = 0, 1
    return np.ascontiguousarray(X * case['x_scale']), y


def direction(case):
    """The rule's unit vector."""
    w = np.random.default_rng([7, case['data_seed'], case['d']]).normal(size=case['d'])
    return w / np.linalg.norm(w)


def job_rows(case):
    """-> [(training rows, held-out rows)], one per seed."""
    n, kind = case['n'], case['jobs']
    rows, extra = np.arange(n), np.arange(n, n + N_VAL)
    if kind == 'all':
        jobs = [(rows, extra) for _ in case['seeds']]
    elif kind == 'empty_middle':
        jobs = [(rows, extra), (np.zeros(0, np.int64), extra), (rows, extra)]
    else:
        k = kind[1]
        jobs = [(rows[rows % k != f], rows[rows % k == f]) for f in range(k)]
        if kind[0] == 'folds+whole':
            jobs.append((rows, extra))
    assert len(jobs) == len(case['seeds'])
    return jobs


def start_weights(case):
    """-> None (the seeded Glorot start) or [(W1, b1, W2, b2)] per job.  'aligned+8' / 'aligned-8': every hidden unit looks along the
    rule's direction with a small positive gain, every output weight is +8 or -8: on rows far from the boundary the units saturate
    with one sign and the output passes +-700."""
    if case['init'] is None:
        return None
    d, h = case['d'], case['hidden']
    rng = np.random.default_rng([11, case['data_seed']])
    gain = rng.uniform(0.05, 0.15, size=h)
    W1 = np.outer(direction(case), gain)
    b1 = rng.uniform(-0.05, 0.05, size=h)
    W2 = np.full(h, {'aligned+8': 8.0, 'aligned-8': -8.0}[case['init']])
    return [(W1, b1, W2, 0.25) for _ in case['seeds']]


def fit_kwargs(case):
    """What Device.mlp_fit and mo.fit both take."""
    return dict(hidden=case['hidden'], batch_size=case['batch_size'], max_iter=case['max_iter'], tol=case['tol'],
                n_iter_no_change=case['n_iter_no_change'], shuffle=case['shuffle'])


def device_fit(dev, case):
    X, y = problem(case)
    return dev.mlp_fit(X, y, job_rows(case), seeds=list(case['seeds']), init=start_weights(case), **fit_kwargs(case))


def _oracle(case):
    X, y = problem(case)
    init = start_weights(case)
    out = []
    for j, (tr, va) in enumerate(job_rows(case)):
        seed = case['seeds'][j]
        if len(tr):
            with np.errstate(over='ignore'):
                want = mo.fit(X[tr], y[tr], seed=seed, init=None if init is None else init[j], **fit_kwargs(case))
        else:                                   # no training rows: the start weights, no epoch
            W1, b1, W2, b2 = init[j] if init is not None else mo.init_weights(case['d'], case['hidden'], seed)
            want = dict(W1=W1, b1=b1, W2=W2, b2=b2, loss_curve=np.zeros(0), n_iter=0)
        with np.errstate(over='ignore'):
            _, p = mo.forward(want['W1'], want['b1'], want['W2'], want['b2'], X[va])
            want['val_correct'] = int(round(mo.accuracy(want, X[va], y[va]) * len(va))) if len(va) else 0
        want['p_val'] = p
        out.append(want)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_by_name(name):
    return _oracle(WORKER_CASE if name == WORKER_CASE['name'] else CASES[name])


def oracle(case):
    """The oracle's fits of the case's jobs, computed once and shared: do not write into them.  Each is mo.fit's dict plus
    val_correct (mo.accuracy's count on the held-out rows) and p_val (its probabilities there)."""
    return _oracle_by_name(case['name'])


def tolerances(n_iter):
    """(loss rtol, weights rtol, weights atol) that tests/test_gpu_train.py states for fits of this length."""
    if n_iter <= 8:
        return 1e-8, 1e-6, 1e-9
    assert n_iter <= 25, 'no tolerance is stated for fits beyond 25 epochs'
    return 1e-7, 1e-5, 1e-7
