"""Worker for tests/test_gpu_xmfa_lift.py::test_hand_made_edges_with_poisoned_allocations: a process of its own, because the
library reads MCALLER_POISON once.  Every hand-made edge of tests/xmfa_cases.py, as it stands and with both strands of every block
flipped, and the file without a paired block, through one context."""
import os
import pathlib
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    from tests import xmfa_cases as X
    assert os.environ.get('MCALLER_POISON') == '1'
    dev, tmp = get_device(), pathlib.Path(sys.argv[1])
    cases = X.edge_cases()
    assert len(cases) == 2 * len(X.edge_block_sets())
    for i, c in enumerate(cases):
        xs, _ = X.device_makes_it(dev, tmp, c, 'e%d.' % i)
        print(c['name'], xs['n_lines'], xs['n_entries'], xs['n_columns'], xs['n_words'], xs['n_mapped'])
    xs, cs = X.device_makes_it(dev, tmp, X.unpaired_case(), 'u.')
    assert xs['n_paired_blocks'] == 0 and xs['n_mapped'] == 0 and cs['n_sites'] == 0 and cs['n_out_bytes'] == 0
    print('edges ok')
