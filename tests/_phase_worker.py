"""Worker for tests/test_gpu_phase_reads.py::test_a_decline_then_clean_calls_with_poisoned_allocations: a process of its own,
because the library reads MCALLER_POISON once.  A file with a duplicate call is declined behind the counters' kernels, then every
case the device is expected to make goes through the same context, with and without q-values."""
import os
import pathlib
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


if __name__ == '__main__':
    from mcaller_amd.device import get_device
    from tests import phase_cases as K
    from tests.test_gpu_phase_reads import device_makes_it, host_does_it
    assert os.environ.get('MCALLER_POISON') == '1'
    dev, tmp = get_device(), pathlib.Path(sys.argv[1])
    text, opt, _ = K.case_shuffled()
    lines = text.decode().splitlines(True)
    host_does_it(dev, tmp, ''.join(lines + [lines[7]]).encode(), opt, 'duplicate', len(lines))
    for name in sorted(K.DEVICE_CASES):
        text, opt, _ = K.DEVICE_CASES[name]()
        for fdr in (False, True):
            fig = device_makes_it(dev, tmp, text, opt, fdr=fdr, threshold=1.0, what=name, files=False)[3]
            print(name, fdr, fig)
    print('phase ok')
