"""Worker for tests/test_gpu_phase_edges.py::test_the_small_cases_with_poisoned_allocations: a process of its own, because the
library reads MCALLER_POISON once.  A duplicate at a site that is not kept is declined behind kr_order, then the small served cases
of tests/phase_edge_cases.py -- the long reads in both arrivals, the near keys, the option and position edges -- go through the same
context, with and without q-values."""
import os
import pathlib
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    from tests import phase_edge_cases as E
    from tests.test_gpu_phase_reads import device_makes_it, host_does_it
    assert os.environ.get('MCALLER_POISON') == '1'
    dev, tmp = get_device(), pathlib.Path(sys.argv[1])
    text, opt, claims = E.case_duplicate('unkept')
    host_does_it(dev, tmp, text, opt, 'duplicate', claims['line'])
    for name in E.SMALL:
        text, opt, _ = E.SERVED[name]()
        for fdr in (False, True):
            fig = device_makes_it(dev, tmp, text, opt, fdr=fdr, threshold=0.0, what=name, files=False)[3]
            print(name, fdr, fig)
    print('phase edges ok')
