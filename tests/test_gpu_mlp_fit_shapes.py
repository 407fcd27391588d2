"""k4_mlp_fit (csrc/mc_train.hip) on every path, width and batch edge it has: the cases of tests/mlp_fit_cases.py, each against
oracle/mlp_fit_oracle.py::fit on the same rows, seeds and parameters (fp64 NumPy, pinned to scikit-learn's runs by
tests/test_train.py).  tests/test_mlp_fit_cases.py checks without a GPU that every case reaches the edge it names.

Per job: n_iter equal, the loss curve, ALL of W1, b1, W2, b2, and val_correct EQUAL to the oracle's count (no held-out row of any case
has p within 1e-4 of 0.5).  Tolerances are the ones tests/test_gpu_train.py states for fits of the same length (MC.tolerances): up to
8 epochs rtol 1e-8 on the loss and rtol 1e-6 / atol 1e-9 on the weights, up to 25 epochs 1e-7 and 1e-5 / 1e-7.  The batch_size=32
stopping case would run to 26 epochs: it is given max_iter=25, so that the 25-epoch tolerances cover it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mlp_fit_oracle as mo
from tests import helpers as H
from tests import mlp_fit_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def worst(got, want):
    """Largest relative error (for printing: a weight near zero makes it large without meaning anything)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def hold(got, want, label):
    """One job of the device against the oracle's fit of it; the figures are printed before anything is asserted."""
    lr, wr, wa = MC.tolerances(want['n_iter'])
    print('%s: n_iter %d / %d, val_correct %d / %d, worst relative error: loss %.2e, W1 %.2e, b1 %.2e, W2 %.2e, b2 %.2e'
          % (label, got['n_iter'], want['n_iter'], got['val_correct'], want['val_correct'], worst(got['loss_curve'], want['loss_curve']),
             worst(got['W1'], want['W1']), worst(got['b1'], want['b1']), worst(got['W2'], want['W2']), worst(got['b2'], want['b2'])))
    assert got['n_iter'] == want['n_iter'], label
    assert got['loss_curve'].shape == want['loss_curve'].shape
    np.testing.assert_allclose(got['loss_curve'], want['loss_curve'], rtol=lr, atol=0, err_msg=label)
    for k in ('W1', 'b1', 'W2', 'b2'):
        assert np.shape(got[k]) == np.shape(want[k])
        np.testing.assert_allclose(got[k], want[k], rtol=wr, atol=wa, err_msg='%s %s' % (label, k))
    assert got['val_correct'] == want['val_correct'], label


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert x['n_iter'] == y['n_iter'] and x['val_correct'] == y['val_correct'] and x['b2'] == y['b2']
        for k in ('W1', 'b1', 'W2', 'loss_curve'):
            assert x[k].tobytes() == y[k].tobytes(), k


@pytest.mark.parametrize('name', sorted(MC.CASES))
def test_case_equals_the_oracle(dev, name):
    case = MC.CASES[name]
    got, want = MC.device_fit(dev, case), MC.oracle(case)
    assert len(got) == len(want) == len(case['seeds'])
    for j in range(len(want)):
        hold(got[j], want[j], '%s job %d' % (name, j))


@pytest.mark.parametrize('name', ['empty_middle_four_wgs', 'empty_middle_one_wg'])
def test_job_without_training_rows_returns_its_start(dev, name):
    """Its start weights exactly as init_weights gives them, no epoch, an empty curve, and the held-out rows counted on those
    weights."""
    case = MC.CASES[name]
    got, want = MC.device_fit(dev, case)[1], MC.oracle(case)[1]
    W1, b1, W2, b2 = mo.init_weights(case['d'], case['hidden'], case['seeds'][1])
    print('%s: start weights that differ from init_weights: W1 %d of %d, b1 %d, W2 %d, b2 %d' % (
        name, (got['W1'] != W1).sum(), W1.size, (got['b1'] != b1).sum(), (got['W2'] != W2).sum(), got['b2'] != b2))
    assert got['n_iter'] == 0 and got['loss_curve'].shape == (0,)
    assert got['W1'].tobytes() == W1.tobytes() and got['b1'].tobytes() == b1.tobytes() and got['W2'].tobytes() == W2.tobytes()
    assert got['b2'] == b2
    assert got['val_correct'] == want['val_correct']


@pytest.mark.parametrize('name', ['width_65_one_wg', 'stop_batch_200', 'stop_batch_32'])
def test_same_call_twice_gives_the_same_bytes(dev, name):
    """(the only place where the device is compared with itself: repeatability is the thing tested)"""
    case = MC.CASES[name]
    same_bytes(MC.device_fit(dev, case), MC.device_fit(dev, case))


def test_both_sides_of_the_switch_on_the_same_rows(dev):
    """batch_size 63 (one workgroup) and 64 (four) on the same 200 rows with the same seed: each agrees with its own oracle run, and
    the two oracle runs differ, because the batches differ."""
    a, b = MC.CASES['batch_63'], MC.CASES['batch_64']
    Xa, ya = MC.problem(a)
    Xb, yb = MC.problem(b)
    assert Xa.tobytes() == Xb.tobytes() and ya.tobytes() == yb.tobytes() and a['seeds'] == b['seeds']
    assert (MC.workgroups(63), MC.workgroups(64)) == (1, 4)
    [wa], [wb] = MC.oracle(a), MC.oracle(b)
    assert np.abs(wa['loss_curve'] - wb['loss_curve']).min() > 1e-6 * wa['loss_curve'].max()
    [ga], [gb] = MC.device_fit(dev, a), MC.device_fit(dev, b)
    hold(ga, wa, 'batch_63')
    hold(gb, wb, 'batch_64')
    assert np.abs(ga['loss_curve'] - gb['loss_curve']).min() > 1e-6 * wa['loss_curve'].max()


def test_refusals_touch_nothing(dev):
    """batch_size 257, hidden 0 and 129 and ten inputs: -12 with the message, through the C ABI, before the device is touched and
    without a byte written to the outputs.  A fit afterwards still works."""
    from mcaller_amd import _lib
    case = MC.CASES['width_65_one_wg']
    X7, y = MC.problem(case)
    n = len(y)
    X10 = np.ascontiguousarray(np.random.default_rng(1).normal(size=(n, 10)))
    L = _lib.lib()
    off = np.array([0, n], np.int64)
    rows = np.arange(n, dtype=np.int32)

    def call(X, hidden=16, batch_size=64):
        d, h = X.shape[1], max(hidden, 1)
        out = dict(W1=np.full((d, h), 7.5), b1=np.full(h, 7.5), W2=np.full(h, 7.5), b2=np.full(1, 7.5), curve=np.full(4, 7.5),
                   n_iter=np.full(1, -3, np.int32), correct=np.full(1, -3, np.int64))
        prm = _lib.FitParams(d, hidden, batch_size, 4, 10, 1, 0.001, 0.001, 0.9, 0.999, 1e-8, 1e-4, 1)
        rc = L.mc_mlp_fit(dev._ctx, C.byref(prm), _lib._ptr(X), _lib._ptr(y), n, 1, _lib._ptr(off), _lib._ptr(rows), _lib._ptr(off),
                          _lib._ptr(rows), None, None, _lib._ptr(out['W1']), _lib._ptr(out['b1']), _lib._ptr(out['W2']), _lib._ptr(out['b2']),
                          _lib._ptr(out['curve']), _lib._ptr(out['n_iter']), _lib._ptr(out['correct']))
        untouched = all((out[k] == 7.5).all() for k in ('W1', 'b1', 'W2', 'b2', 'curve')) and out['n_iter'][0] == -3 and out['correct'][0] == -3
        return rc, L.mc_last_error(), untouched, out

    rc, msg, untouched, _ = call(X7, batch_size=257)
    assert rc == -12 and b'mc_mlp_fit: batch size 257 does not fit (max 256 rows)' in msg and untouched
    for X, hidden in ((X7, 0), (X7, 129), (X10, 16)):
        rc, msg, untouched, _ = call(X, hidden=hidden)
        assert rc == -12 and b'mc_mlp_fit: unsupported shape (inputs 1..9, hidden 1..128)' in msg and untouched
    rc, msg, untouched, out = call(X7, batch_size=256)
    assert rc == 0 and not untouched and out['n_iter'][0] == 4
    hold(MC.device_fit(dev, case)[0], MC.oracle(case)[0], 'after the refusals')


def test_group_sizes_in_processes_of_their_own(tmp_path):
    """MCALLER_FIT_WGS = 1, 2 and 8 (read once per process): tests/_mlp_fit_worker.py in a fresh child for each, one after the other
    (never two with the GPU open), each with a time limit; each held against the oracle with the 25-epoch tolerances.  A child that
    fails or runs out of time fails the test there: no further child is started."""
    case = MC.WORKER_CASE
    want = MC.oracle(case)
    assert MC.tolerances(case['max_iter']) == (1e-7, 1e-5, 1e-7)
    for wgs in (1, 2, 8):
        path = str(tmp_path / ('fits_%d.npz' % wgs))
        env = dict(os.environ, MCALLER_FIT_WGS=str(wgs), PYTHONPATH=H.REPO)
        done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_mlp_fit_worker.py'), path], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, timeout=120)
        assert done.returncode == 0 and b'fits written: 6' in done.stdout, done.stdout.decode('utf-8', 'replace')[-2000:]
        z = np.load(path)
        for j in range(len(want)):
            got = {k: z['%s_%d' % (k, j)] for k in ('W1', 'b1', 'W2', 'loss_curve')}
            got.update(b2=float(z['b2_%d' % j]), n_iter=int(z['n_iter_%d' % j]), val_correct=int(z['val_correct_%d' % j]))
            hold(got, want[j], 'MCALLER_FIT_WGS=%d job %d' % (wgs, j))
