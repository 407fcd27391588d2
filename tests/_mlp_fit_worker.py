"""Worker for tests/test_gpu_mlp_fit_shapes.py::test_group_sizes_in_processes_of_their_own: a process of its own, because the library
reads MCALLER_FIT_WGS once.  The product's shape (six fits, 100 hidden units, batches of 200, 12 epochs) through Device.mlp_fit; the
results go to the .npz named on the command line, the caller holds them against the oracle."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(dev, path):
    import numpy as np
    from tests import mlp_fit_cases as MC
    got = MC.device_fit(dev, MC.WORKER_CASE)
    out = {}
    for j, g in enumerate(got):
        for k in ('W1', 'b1', 'W2', 'b2', 'loss_curve', 'n_iter', 'val_correct'):
            out['%s_%d' % (k, j)] = np.asarray(g[k])
    np.savez(path, **out)
    return len(got)


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    assert int(os.environ['MCALLER_FIT_WGS']) >= 1
    print('fits written: %d' % run(get_device(), sys.argv[1]))
