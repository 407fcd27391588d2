"""mc_twosample.h's host build (mc_twosample: _lib.twosample) against the SciPy calls of compare_genomes' definition: U and D bit for
bit, every rounded value equal as text or the status naming why it is not vouched for; the degenerate cases; the committed grid
against profiles/twosample_error.json.  Needs no GPU."""
import json
import os

import numpy as np
import pytest

from mcaller_amd import _lib
from tests import helpers as H
from tests import twosample_cases as T
from tests import twosample_grid as G

KNOWN_BITS = 0
for _bit in _lib.TW_STATUS.values():
    KNOWN_BITS |= _bit

CASES = T.seeded() + T.seeded(T.HOST_ONLY_SIZES)


@pytest.fixture(scope='module')
def results():
    """name -> (status, values, bounds, the statement's text): computed once."""
    return {name: _lib.twosample(x, y) + (T.statement_text(x, y),) for name, x, y in CASES}


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_host_build_against_scipy(results, name):
    st, out, bound, want = results[name]
    got = T.text_of(out)
    print(name, st, got, want, bound.tolist())
    assert st & ~KNOWN_BITS == 0
    assert not st & (_lib.TW_STATUS['bad_n'] | _lib.TW_STATUS['deep'] | _lib.TW_STATUS['no_convergence'])
    if not st & (_lib.TW_STATUS['all_equal'] | _lib.TW_STATUS['zero_var']):
        assert np.float64(want[0]).tobytes() == np.float64(out[0]).tobytes()           # U
        assert np.float64(want[4]).tobytes() == np.float64(out[4]).tobytes()           # D
        assert got[0] == want[0] and got[4] == want[4]
    if st == 0:
        assert got == want
        assert np.all(bound >= 0.0) and np.all(np.isfinite(bound))


def test_most_sites_are_vouched_for(results):
    """The tie test declines a value on a rounding tie, not as a habit: nine sites in ten of the seeded set stand."""
    vouched = sum(1 for st, _, _, _ in results.values() if st == 0)
    print(vouched, len(results), {n: r[0] for n, r in results.items() if r[0]})
    assert vouched * 10 >= len(results) * 9


def test_unvouched_values_are_near_ties_only(results):
    """A status of `tie` alone still carries values, and they differ from the statement's by a thousandth at the most."""
    for name, (st, out, bound, want) in results.items():
        if st == _lib.TW_STATUS['tie']:
            for g, w in zip(out, want):
                assert abs(float(g) - float(w)) <= 0.001 + 1e-12, (name, g, w)


@pytest.mark.parametrize('name', sorted(T.DEGENERATE))
def test_degenerate_cases_name_their_status(name):
    x, y, status = T.DEGENERATE[name]
    st, out, bound = _lib.twosample(x, y)
    print(name, st, out.tolist())
    assert st & _lib.TW_STATUS[status], (name, st)
    if status == 'far_tail':
        want = T.statement_text(x, y)
        assert T.text_of(out)[0] == want[0] and T.text_of(out)[4] == want[4]


def test_identical_samples():
    x, _ = T.sample('round2', 20, 25, 3)
    st, out, bound = _lib.twosample(x, x)
    want = T.statement_text(x, x)
    assert out[0] == len(x) * len(x) / 2 and out[4] == 0.0
    assert want[0] == repr(len(x) * len(x) / 2) and want[4] == '0.0' and want[5:] == ['0.0'] * 4
    if st == 0:
        assert T.text_of(out) == want
    else:                                                   # (t = 0 within its bound of -0.0: the sign of the printed zero)
        assert st == _lib.TW_STATUS['tie'] and T.text_of(out)[5:] == ['0.0'] * 4


def test_grid_reproduces_the_profile():
    doc = json.load(open(os.path.join(H.REPO, 'profiles', 'twosample_error.json')))
    m = G.measure()
    print(m)
    assert doc['bound'] == G.FN_BOUND
    assert G.FN_BOUND >= 64 * doc['measured_max'] and G.FN_BOUND <= 128 * doc['measured_max']      # (x 64, rounded up -- not further)
    assert m['normal']['points'] == doc['normal']['points'] and m['kolmogorov']['points'] == doc['kolmogorov']['points']
    for got in (m['normal']['max_vs_sf'], m['normal']['max_vs_logsf'], m['kolmogorov']['max']):
        assert got <= G.FN_BOUND
    # the grid reaches where log10 p reaches -290
    z, by_sf, _ = G.normal_grid()
    lam, l = G.kolmogorov_grid()
    assert by_sf.min() < -285.0 and l.min() < -285.0


def test_header_and_grid_agree_on_the_bound():
    src = open(os.path.join(H.REPO, 'mcaller_amd', 'csrc', 'mc_twosample.h')).read()
    assert '#define TW_FN_BOUND %s ' % ('%.1e' % G.FN_BOUND) in src


def test_gpu_generator_has_no_declined_site():
    """The condition of tests/test_gpu_compare.py: where it demands by == 'device', the seeded sites are vouched for by the host
    build of the header (no degenerate site, no rounding tie).  A device decline there is then a failure."""
    from tests import gpu_compare_cases as GC
    for what, sites in GC.device_site_sets().items():
        bad = [(i, _lib.twosample(x, y)[0]) for i, (x, y) in enumerate(sites)]
        bad = [b for b in bad if b[1] != 0]
        assert not bad, (what, bad)
