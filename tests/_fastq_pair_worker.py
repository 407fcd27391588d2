"""Worker for tests/test_gpu_fastq.py::test_two_calls_in_a_row_with_poisoned_allocations: a process of its own, because the library reads
MCALLER_POISON once.  A large text and then a small one through one context, each against the record rules on the CPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pair(dev):
    import numpy as np
    from mcaller_amd import _lib
    from tests import fastq_cases as F
    large = F.random_fastq(np.random.default_rng(5), 3000, crlf=True)
    small = b'@a\nAC\n+\nI5\n@b_1\n\n+\n\n'
    for text in (large, small, large, small):
        keys, means, reason = dev.fastq_qualities(text=text)
        assert reason is None, reason
        hk, hm, decline = _lib.fastq_records_host(text)
        assert decline is None and keys == hk and means.tobytes() == hm.tobytes()
    assert len(keys) == 2


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    assert os.environ.get('MCALLER_POISON') == '1'
    pair(get_device())
    print('pair ok')
