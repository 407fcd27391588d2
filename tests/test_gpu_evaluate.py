"""The arithmetic of mcaller_amd.evaluate on the GPU: mc_hypergeom.h's device build (mc_hypergeom_tail_device, a lane per case)
against exact rationals and against the host build, on the grid of tests/test_hypergeom.py in one launch."""
import numpy as np
import pytest

from tests import hypergeom_grid as G

pytestmark = pytest.mark.gpu


def test_device_tail_against_exact_rationals_and_the_host_build():
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    N, K, d, k, exact = G.cases()
    assert len(N) > 15000
    tail, err = get_device().hypergeom_tail(N, K, d, k)                    # one launch
    worst = 0.0
    for i, (num, den) in enumerate(exact):
        assert G.within(tail[i], err[i], num, den), (N[i], K[i], d[i], k[i], tail[i], err[i])
        worst = max(worst, G.abs_error(tail[i], num, den))
    print('largest |device tail - exact| %.3g; largest derived bound %.3g' % (worst, err.max()))
    assert err.max() < 2e-12 and (tail >= 0.0).all() and (tail <= 1.0).all()
    # the host build lies within the SUM of the two bounds (both are within their own of the exact tail); the trivial cases agree exactly
    h_tail, h_err = _lib.hypergeom_tail(N, K, d, k)
    assert (np.abs(tail - h_tail) <= err + h_err).all()
    trivial = h_err == 0.0
    assert trivial.any() and (tail[trivial] == h_tail[trivial]).all() and (err[trivial] == 0.0).all()


def test_device_tail_bad_arguments_and_an_empty_call():
    from mcaller_amd.device import get_device
    dev = get_device()
    tail, err = dev.hypergeom_tail([5, 5, (1 << 31) - 1], [6, 2, 1000], [1, 2, 1024], [1, 1, 1])
    assert np.isnan(tail[0]) and np.isnan(err[0])
    assert abs(tail[1] - 0.7) <= err[1] < 1e-14
    num, den = G.tail_numerators((1 << 31) - 1, 1000, 1024)
    assert G.within(tail[2], err[2], num[1], den)
    assert dev.hypergeom_tail([], [], [], [])[0].shape == (0,)
    with pytest.raises(ValueError):
        dev.hypergeom_tail([1, 2], [1], [1], [1])

