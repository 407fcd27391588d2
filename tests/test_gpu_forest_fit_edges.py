"""k5_forest_fit and k5_forest_val (csrc/mc_forest_fit.hip) on the paths tests/test_gpu_forest_fit.py leaves unrun: levels wider than
one workgroup, batches, the tile edges of the two block scans, ties, the 1e-7 rule, jobs that hardly are any, validation values on
a threshold.  The cases are tests/forest_fit_cases.py's; tests/test_forest_fit_cases.py shows without a GPU that each reaches its
path.  Every result is held against tests/forest_fit_oracle.py::fit_jobs as assert_same_forest does: every field of every node byte
for byte, val_correct equal.  No tolerance anywhere."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import forest_fit_cases as FC
from tests import forest_fit_oracle as fo
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize('name', FC.NAMES)
def test_case_equals_the_oracle(dev, name):
    c, want = FC.case(name), FC.oracle(name)
    t0 = time.perf_counter()
    got = FC.device_fit(dev, name)
    print('%s: %.3f s on the device' % (name, time.perf_counter() - t0))
    FC.assert_same_jobs(got, want, c['jobs'])
    st = dev.forest_fit_last_stats()
    total = len(c['jobs']) * c['prm']['n_trees']
    assert (st['n_batches'], st['batch'], st['n_trees_total']) == (1, total, total)
    assert st['n_nodes'] == sum(len(t['left']) for w in want for t in w['trees']) and st['per_tree_bytes'] > 9 * len(c['X'])


def test_validation_rows_on_thresholds_scored_by_k3_forest_too(dev):
    """The forest of the on_thresholds case through set_classifier / classifier_forward: fo.predict_proba's bits on the validation rows,
    966 of which carry a value equal to a threshold on their way down."""
    from mcaller_amd.model_io import forest_from_arrays
    c = FC.case('on_thresholds')
    trees = FC.oracle('on_thresholds')[0]['trees']
    got = FC.device_fit(dev, 'on_thresholds')[0]
    FC.assert_same_forest(got, trees)
    Xv = c['X'][c['jobs'][0][1]]
    w = forest_from_arrays(got['tree_off'], got['left'], got['right'], got['feature'], got['threshold'], got['value'], 7)
    dev.set_classifier([w], np.zeros(256, dtype=np.uint8))
    p = dev.classifier_forward(Xv, np.zeros(len(Xv), dtype=np.uint8))
    P0, P1 = fo.predict_proba(trees, Xv)
    assert (np.asarray(p).view(np.uint8) == P1.view(np.uint8)).all()
    assert got['val_correct'] == int(((P1 > P0) == (c['y'][c['jobs'][0][1]] == 1)).sum())


def megabytes_for(batch, per_tree, total):
    """A whole MCALLER_FOREST_MEM_MB at which `batch` trees of per_tree bytes fit and batch + 1 do not (or all `total` fit)."""
    for mb in range(1, (((total + 2) * per_tree) >> 20) + 4):
        if max(1, min(total, (mb << 20) // per_tree)) == batch:
            return mb
    raise AssertionError('no whole number of MB gives batches of %d trees at %d bytes a tree' % (batch, per_tree))


def test_batches_in_processes_of_their_own(dev, tmp_path):
    """MCALLER_FOREST_MEM_MB (read once per process) such that the 14 trees grow 1, 4 and 14 at a time: tests/_forest_fit_worker.py in a
    fresh child for each, one after the other (never two at once), each with a time limit.  A batch of 4 ends with a batch of 2 and
    its second batch crosses from job 0 to job 1.  Every child's forests equal the oracle's, hence each other's; the stats say how
    the call was cut.  A child that fails or runs out of time fails the test there: no further child is started."""
    c, want = FC.case(FC.WORKER_CASE), FC.oracle(FC.WORKER_CASE)
    FC.assert_same_jobs(FC.device_fit(dev, FC.WORKER_CASE), want, c['jobs'])           # unbatched, in this process
    st = dev.forest_fit_last_stats()
    n_nodes = sum(len(t['left']) for w in want for t in w['trees'])
    assert (st['n_batches'], st['batch'], st['n_trees_total'], st['n_nodes']) == (1, 14, 14, n_nodes)
    per_tree = st['per_tree_bytes']
    assert per_tree > 0
    for batch, n_batches in ((1, 14), (4, 4), (14, 1)):
        mb = megabytes_for(batch, per_tree, 14)
        path = str(tmp_path / ('forest_%d.npz' % batch))
        env = dict(os.environ, MCALLER_FOREST_MEM_MB=str(mb), PYTHONPATH=H.REPO)
        done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_forest_fit_worker.py'), path], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert done.returncode == 0 and b'jobs written: 2' in done.stdout, done.stdout.decode('utf-8', 'replace')[-2000:]
        z = np.load(path)
        stats = {k: int(z['stat_' + k]) for k in st}
        assert (stats['batch'], stats['n_batches']) == (batch, n_batches), (mb, stats)
        assert (stats['per_tree_bytes'], stats['n_trees_total'], stats['n_nodes']) == (per_tree, 14, n_nodes)
        got = [dict({k: z['%s_%d' % (k, j)] for k in FC.FIELDS + ('tree_off',)}, val_correct=int(z['val_correct_%d' % j]),
                    n_val=int(z['n_val_%d' % j])) for j in range(2)]
        FC.assert_same_jobs(got, want, c['jobs'])
