"""Worker for tests/test_gpu_textfeed.py::test_every_pipeline_in_turn_with_poisoned_allocations: a process of its own, because the
library reads MCALLER_POISON once.  The four file pipelines in turn through one context's shared stages, in blocks of 256 bytes
(tests/textfeed_cases.mixed)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    from tests import textfeed_cases as C
    assert os.environ.get('MCALLER_POISON') == '1' and os.environ.get(C.KNOB) == '256'
    C.mixed(get_device(), sys.argv[1])
    print('mixed ok')
