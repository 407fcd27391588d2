"""Worker for tests/test_gpu_forest_fit_edges.py::test_batches_in_processes_of_their_own: a process of its own, because the library
reads MCALLER_FOREST_MEM_MB once.  Two jobs of 7 trees on 4000 rows (tests/forest_fit_cases.py: WORKER_CASE) through
Device.forest_fit; the arrays and the call's mc_forest_fit_stats go to the .npz named on the command line, the caller holds them
against the oracle."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(dev, path):
    import numpy as np
    from tests import forest_fit_cases as FC
    got = FC.device_fit(dev, FC.WORKER_CASE)
    out = {'stat_' + k: np.asarray(v) for k, v in dev.forest_fit_last_stats().items()}
    for j, g in enumerate(got):
        for k in FC.FIELDS + ('tree_off', 'val_correct', 'n_val'):
            out['%s_%d' % (k, j)] = np.asarray(g[k])
    np.savez(path, **out)
    return len(got)


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    assert int(os.environ['MCALLER_FOREST_MEM_MB']) >= 1
    print('jobs written: %d' % run(get_device(), sys.argv[1]))
