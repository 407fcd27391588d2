"""mc_decimal.h, the device build (Device.parse_doubles -> mc_parse_doubles_device, a lane per token): the bits of float(), the
declines, and token by token the verdict of the host build, in calls of 1, 63, 64, 65 and 10^5 tokens (below, at and above a
wave; many workgroups).  Every call's last token ends at the last byte of the text; tokens of 1 and of 30 bytes are among them."""
import numpy as np
import pytest

from tests import decimal_cases as D

pytestmark = pytest.mark.gpu

CALLS = (1, 63, 64, 65, 100000)


@pytest.fixture(scope='module')
def tokens():
    """The declines and the shapes first (so that the small calls hold them too), then the half-way cases, repr()s and %de%d."""
    fixed = ['5', '.', '00000000000000000000001.500000', '0.0000000000000000000000000015']
    assert [len(t) for t in fixed] == [1, 1, 30, 30]
    toks = fixed + list(D.set_e()) + list(D.set_d()[:40]) + list(D.set_c()) + list(D.set_d()[40:]) + list(D.set_a()) + list(D.set_b())
    assert len(toks) >= sum(CALLS)
    return [t.encode('latin-1') for t in toks[:sum(CALLS)]]


@pytest.fixture(scope='module')
def host_verdicts(tokens):
    from mcaller_amd import _lib
    return [_lib.parse_double(t) for t in tokens]


def test_device_equals_float_and_the_host_build(tokens, host_verdicts):
    from mcaller_amd.device import get_device
    dev = get_device()
    at, seen_declined, seen_parsed = 0, 0, 0
    for n in CALLS:
        chunk, host = tokens[at:at + n], host_verdicts[at:at + n]
        at += n
        out, ok = dev.parse_doubles(chunk)
        assert len(out) == len(ok) == n
        host_ok = np.array([h is not None for h in host])
        assert (ok == host_ok).all(), [chunk[i] for i in np.nonzero(ok != host_ok)[0][:5]]
        want = np.array([float(t.decode('latin-1')) if h is not None else 0.0 for t, h in zip(chunk, host)], dtype=np.float64)
        same = out.view(np.uint64) == want.view(np.uint64)
        assert same.all(), [(chunk[i], out[i], want[i]) for i in np.nonzero(~same)[0][:5]]
        seen_declined += int((~ok).sum())
        seen_parsed += int(ok.sum())
    assert seen_declined >= len(D.set_e()) and seen_parsed > 90000


def test_declines_and_in_range_strings_on_the_device():
    from mcaller_amd.device import get_device
    dev = get_device()
    _, ok = dev.parse_doubles([s.encode('latin-1') for s in D.set_e()])
    assert not ok.any(), [s for s, o in zip(D.set_e(), ok) if o]
    inside = [s for s in D.set_c() + D.set_d() if D.in_range(s)]
    out, ok = dev.parse_doubles([s.encode('latin-1') for s in inside])
    assert ok.all(), [s for s, o in zip(inside, ok) if not o][:5]
    assert [D.bits(v) for v in out.tolist()] == [D.bits(float(s)) for s in inside]
    out, ok = dev.parse_doubles([])
    assert len(out) == 0 and len(ok) == 0
