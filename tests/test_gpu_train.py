"""The HIP fit kernel (mc_mlp_fit) against the CPU restatement of scikit-learn's optimiser (oracle/mlp_fit_oracle.py,
itself pinned against scikit-learn runs) and against the committed scikit-learn golden vectors.  fp64 on both sides, but
tanh/exp/log and the summation order differ in the last bits and Adam amplifies that slowly: tolerances are stated."""
import json
import os

import numpy as np
import pytest

from oracle import mlp_fit_oracle as mo
from tests import helpers as H

pytestmark = pytest.mark.gpu
TRAIN = os.path.join(H.GOLDEN, 'train')
MANIFEST = json.load(open(os.path.join(TRAIN, 'manifest.json')))


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize('tag', sorted(MANIFEST['fits']))
def test_fit_from_given_start_equals_sklearn(dev, tag):
    """scikit-learn's own run (same start weights, shuffle=False): loss curve to 1e-6 relative, same epoch count
    (stopping rule), weights to 1e-4, probabilities to 1e-5 (the north star's tolerance on p)."""
    meta = MANIFEST['fits'][tag]
    z = np.load(os.path.join(TRAIN, tag + '.npz'))
    n = len(z['y'])
    init = [(z['W1_0'], z['b1_0'], z['W2_0'], float(z['b2_0'][0]))]
    got = dev.mlp_fit(z['X'], z['y'], [(np.arange(n), np.arange(n))], hidden=meta['hidden'], max_iter=meta['max_iter'],
                      shuffle=False, init=init)[0]
    assert got['n_iter'] == meta['n_iter']
    np.testing.assert_allclose(got['loss_curve'], z['loss_curve'], rtol=1e-6)
    np.testing.assert_allclose(got['W1'], z['W1'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got['W2'], z['W2'], rtol=1e-4, atol=1e-6)
    _, p = mo.forward(got['W1'], got['b1'], got['W2'], got['b2'], z['X'])
    np.testing.assert_allclose(p, z['proba'], atol=1e-5)
    assert got['val_correct'] == int(round(float(z['train_accuracy'][0]) * n))


def test_seeded_fits_equal_the_oracle(dev):
    """Our start weights and epoch shuffles (the parts scikit-learn leaves to random_state=None): several jobs at once,
    train/validation splits, a short last batch."""
    z = np.load(os.path.join(TRAIN, 'n1000_h100.npz'))
    X, y = z['X'], z['y']
    fold = np.arange(len(y)) % 5
    jobs = [(np.nonzero(fold != f)[0], np.nonzero(fold == f)[0]) for f in range(5)] + [(np.arange(len(y)), np.zeros(0, np.int64))]
    seeds = [11, 12, 13, 14, 15, 99]
    got = dev.mlp_fit(X, y, jobs, hidden=100, max_iter=25, seeds=seeds)
    for j, (tr, va) in enumerate(jobs):
        want = mo.fit(X[tr], y[tr], hidden=100, max_iter=25, seed=seeds[j])
        assert got[j]['n_iter'] == want['n_iter'] == 25
        np.testing.assert_allclose(got[j]['loss_curve'], want['loss_curve'], rtol=1e-7)
        for k in ('W1', 'b1', 'W2', 'b2'):
            np.testing.assert_allclose(got[j][k], want[k], rtol=1e-5, atol=1e-7, err_msg=k)
        if len(va):
            assert abs(got[j]['val_correct'] - round(mo.accuracy(want, X[va], y[va]) * len(va))) <= 1
            assert got[j]["val_correct"] > 0.6 * len(va)          # better than chance after 25 epochs


def test_small_shapes(dev):
    rng = np.random.default_rng(3)
    for n, d, h in [(1, 7, 100), (5, 3, 4), (201, 9, 128), (64, 2, 1)]:
        X = rng.normal(size=(n, d))
        y = (rng.random(n) < 0.5).astype(np.uint8)
        got = dev.mlp_fit(X, y, [(np.arange(n), np.arange(n))], hidden=h, max_iter=8, seed=5)[0]
        want = mo.fit(X, y, hidden=h, max_iter=8, seed=5)
        np.testing.assert_allclose(got['loss_curve'], want['loss_curve'], rtol=1e-8)
        np.testing.assert_allclose(got['W2'], want['W2'], rtol=1e-6, atol=1e-9)


def test_more_fits_than_xcds_and_repeatability(dev):
    """Eleven fits in one call (more than the eight a launch spreads over the XCDs one per XCD: the plain numbering of a fit's
    workgroups) against the oracle, and the same call again: the workgroups of a fit add their sums in a fixed order, so a repeated
    call gives the same bytes whichever workgroup arrived first."""
    z = np.load(os.path.join(TRAIN, 'n1000_h100.npz'))
    X, y = z['X'], z['y']
    n = len(y)
    jobs = [(np.nonzero(np.arange(n) % 11 != f)[0], np.nonzero(np.arange(n) % 11 == f)[0]) for f in range(11)]
    seeds = list(range(21, 32))
    got = dev.mlp_fit(X, y, jobs, hidden=100, max_iter=12, seeds=seeds)
    again = dev.mlp_fit(X, y, jobs, hidden=100, max_iter=12, seeds=seeds)
    for j in (0, 5, 10):
        want = mo.fit(X[jobs[j][0]], y[jobs[j][0]], hidden=100, max_iter=12, seed=seeds[j])
        np.testing.assert_allclose(got[j]['loss_curve'], want['loss_curve'], rtol=1e-7)
        for k in ('W1', 'b1', 'W2', 'b2'):
            np.testing.assert_allclose(got[j][k], want[k], rtol=1e-5, atol=1e-7, err_msg=k)
    for j in range(11):
        assert np.array_equal(got[j]['W1'], again[j]['W1']) and np.array_equal(got[j]['loss_curve'], again[j]['loss_curve'])
        assert all(np.array_equal(got[j][k], again[j][k]) for k in ('b1', 'W2', 'b2'))
    # (the library reads MCALLER_FIT_WGS once per process: one workgroup per fit, the switch at batch_size 64 and the group sizes 1, 2
    # and 8 under that variable, in processes of their own, are in tests/test_gpu_mlp_fit_shapes.py; the build macro MC_FIT_GROUPS
    # is exercised by tools/config5.py runs only -- profiles/README.md)


def test_bad_parameters_raise_and_never_fault(dev):
    """What mc_mlp_fit refuses, it refuses before it touches the device (-12 and a message, through the C ABI): a NULL pointer, an
    index outside the matrix, a hidden width beyond two units per lane.  A fit afterwards still works."""
    import ctypes as C
    from mcaller_amd import _lib
    z = np.load(os.path.join(TRAIN, 'n1000_h100.npz'))
    X, y = np.ascontiguousarray(z['X'][:200], dtype=np.float64), np.ascontiguousarray(z['y'][:200], dtype=np.uint8)
    n, d, H_ = len(y), X.shape[1], 16
    L = _lib.lib()
    off = np.array([0, n], np.int64)
    rows = np.arange(n, dtype=np.int32)
    out = dict(W1=np.zeros((d, H_)), b1=np.zeros(H_), W2=np.zeros(H_), b2=np.zeros(1), curve=np.zeros(4), n_iter=np.zeros(1, np.int32),
               correct=np.zeros(1, np.int64))

    def call(hidden=H_, train_off=off, train_idx=rows, val_idx=rows):
        prm = _lib.FitParams(d, hidden, 200, 4, 10, 1, 0.001, 0.001, 0.9, 0.999, 1e-8, 1e-4, 1)
        ptr = lambda a: None if a is None else _lib._ptr(a)                        # noqa: E731
        rc = L.mc_mlp_fit(dev._ctx, C.byref(prm), _lib._ptr(X), _lib._ptr(y), n, 1, ptr(train_off), ptr(train_idx), _lib._ptr(off),
                          ptr(val_idx), None, None, _lib._ptr(out['W1']), _lib._ptr(out['b1']), _lib._ptr(out['W2']), _lib._ptr(out['b2']),
                          _lib._ptr(out['curve']), _lib._ptr(out['n_iter']), _lib._ptr(out['correct']))
        return rc, L.mc_last_error()

    rc, msg = call(train_off=None)
    assert rc == -12 and b'mc_mlp_fit: a required pointer is NULL' in msg
    rc, msg = call(val_idx=None)
    assert rc == -12 and b'mc_mlp_fit: a required pointer is NULL' in msg
    bad = rows.copy()
    bad[7] = n
    rc, msg = call(train_idx=bad)
    assert rc == -12 and b'mc_mlp_fit: row index out of range' in msg
    bad[7] = -1
    rc, msg = call(val_idx=bad)
    assert rc == -12 and b'mc_mlp_fit: row index out of range' in msg
    rc, msg = call(hidden=129)
    assert rc == -12 and b'mc_mlp_fit: unsupported shape' in msg
    rc, msg = call()
    assert rc == 0 and out['n_iter'][0] == 4 and np.isfinite(out['W1']).all() and np.abs(out['W1']).max() > 0
    assert 0 <= out['correct'][0] <= n
    again = dev.mlp_fit(X, y, [(rows, rows)], hidden=H_, max_iter=4, seed=1)[0]
    assert (again['W1'] == out['W1']).all() and again['val_correct'] == out['correct'][0]
