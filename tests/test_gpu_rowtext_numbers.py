"""The GPU row writer's numbers (mc_rowtext.hip, mc_rowtext.h built for gfx950) against Python, byte for byte: the digit kernel
k_rt_digits on arbitrary doubles (as wide slot means and as read qualities), the packed digits unpacked and written through the rows'
own sinks -- RtStoreWords at every start alignment, RtCountRows for the length -- and the integer slot means and probabilities the same
way (mc_ctx_rowtext_probe).  Each item must read as repr(v) / repr(d / 1e4) / str(np.round(p, 2)), be counted as long as it is written,
leave every byte around it as it was, and be refused exactly when the row writer cannot print it."""
import functools
import random

import numpy as np
import pytest

from tests import rowtext_values as RV

pytestmark = pytest.mark.gpu

SHIFTS = (0, 3)                 # two start alignments for every item: (i + 0) % 8 and (i + 3) % 8


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def check_items(dev, got, want, shift, values, what):
    """got: the probe's (text, len, ok); want: the expected text of each item (bytes, or None: refused)."""
    text, length, ok = got
    stride, fill = dev.ROWTEXT_PROBE_STRIDE, dev.ROWTEXT_PROBE_FILL
    n = len(want)
    assert text.shape == (n, stride)
    want_ok = np.array([w is not None for w in want])
    bad = np.nonzero(ok != want_ok)[0]
    assert len(bad) == 0, '%s: ok bit wrong for %d items, first %r (device says %s)' % (what, len(bad), values[bad[0]], bool(ok[bad[0]]))
    lens = np.array([len(w) if w is not None else 0 for w in want], dtype=np.int64)
    want_len = np.where(want_ok, lens, -1)
    bad = np.nonzero(length != want_len)[0]
    assert len(bad) == 0, '%s: counted length wrong for %d items, first %r: %d, written %r' % (
        what, len(bad), values[bad[0]], length[bad[0]], want[bad[0]])
    # the expected 48-byte lines: the fill byte everywhere but each item's own span
    starts = np.arange(n, dtype=np.int64) * stride + (np.arange(n, dtype=np.int64) + shift) % 8
    before = np.concatenate([[0], np.cumsum(lens)[:-1]])
    src = np.frombuffer(b''.join(w for w in want if w), dtype=np.uint8)
    exp = np.full(n * stride, fill, dtype=np.uint8)
    exp[np.repeat(starts - before, lens) + np.arange(len(src))] = src
    bad = np.nonzero((text != exp.reshape(n, stride)).any(axis=1))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError('%s: %d of %d items differ; first %r at alignment %d: want %r, got line %r' % (
            what, len(bad), n, values[i], (i + shift) % 8, want[i], bytes(text[i])))


@functools.lru_cache(maxsize=None)
def double_sets():
    rng = np.random.default_rng(2027)
    sets = {
        'shared': np.array(RV.shortest_values(random.Random(17)), dtype=np.float64),
        'windows': RV.branch_windows(4096),
        'slot_means': RV.slot_mean_values(rng),
        'layouts': RV.layout_values(rng),
        'seventeen': RV.seventeen_digit_values(rng),
        'digit_runs': RV.digit_run_values(rng),
        'patterns': RV.random_patterns(rng),
    }
    return sets


@functools.lru_cache(maxsize=None)
def expected_doubles(name):
    v = double_sets()[name]
    pr = RV.printable(v)
    return [repr(x).encode() if p else None for x, p in zip(v.tolist(), pr.tolist())]


@pytest.mark.parametrize('shift', SHIFTS)
@pytest.mark.parametrize('name', ['shared', 'windows', 'slot_means', 'layouts', 'seventeen', 'digit_runs', 'patterns'])
def test_digits_on_the_device_are_repr(dev, name, shift):
    v = double_sets()[name]
    want = expected_doubles(name)
    got = dev.rowtext_probe(values=v, shift=shift)
    check_items(dev, got, want, shift, v, name)
    if name == 'patterns':
        # the refusals are the host build's too (mc_repr_double_rowtext), pattern by pattern
        from mcaller_amd._lib import repr_double_rowtext
        host_ok = np.array([repr_double_rowtext(x) is not None for x in v.tolist()])
        assert (host_ok == got[2]).all()
        assert 0 < host_ok.sum() < len(v) // 2


def test_value_sets_reach_every_branch():
    """The sets above reach what they are meant to: both digit-generation widths, the exponent form, 17 digits, decpt >= nd."""
    sets = double_sets()
    allv = np.concatenate([sets[k] for k in sets])
    allv = allv[RV.printable(allv) & (allv != 0.0)]
    a = np.abs(allv)
    assert (a < 1e-3).sum() > 500000 and (a >= 1e-3).sum() > 500000
    assert len(sets['slot_means']) >= 10 ** 6
    reprs = [repr(x) for x in sets['layouts'].tolist()]
    assert any('e-' in r for r in reprs) and any(r.endswith('0.0') and len(r) >= 9 for r in reprs)
    for dp in range(-28, 10):
        assert ((a >= 10.0 ** (dp - 1)) & (a < 10.0 ** dp)).any(), dp
    assert len(sets['seventeen']) >= 10000


@functools.lru_cache(maxsize=None)
def fixed_set():
    d = RV.fixed4_values(np.random.default_rng(31))
    return d, [repr(x / 1e4).encode() for x in d.tolist()]


@pytest.mark.parametrize('shift', SHIFTS)
def test_fixed_point_slot_means_on_the_device_are_repr(dev, shift):
    d, want = fixed_set()
    assert len(d) > 5 * 10 ** 6
    check_items(dev, dev.rowtext_probe(fixed=d, shift=shift), want, shift, d, 'fixed4')


@functools.lru_cache(maxsize=None)
def prob_set():
    p = RV.prob_values(np.random.default_rng(37))
    return p, [str(np.round(np.float64(x), 2)).encode() for x in p.tolist()]


@pytest.mark.parametrize('shift', SHIFTS)
def test_probabilities_on_the_device_are_numpys_round(dev, shift):
    p, want = prob_set()
    assert len(p) > 10 ** 6
    check_items(dev, dev.rowtext_probe(prob=p, shift=shift), want, shift, p, 'prob2')


def test_items_of_every_kind_in_one_call(dev):
    """Numbers, integers and probabilities side by side (item numbers run on across the three): wide slot means and qualities that
    are refused sit between printed ones; a probability outside [0, 1] is refused and writes nothing."""
    v = np.array([0.1 + 0.2, float('nan'), 1e-29, 9.999999999999999e-30, -1e9, 999999999.9999999, float('inf'), -0.0, 1.850371707708594e-17])
    d = np.array([-2 ** 31, 0, 70000, -7055], dtype=np.int32)
    p = np.array([0.285, float('nan'), -0.01, 1.01, 1.0, 0.0])
    want = [repr(x).encode() if ok else None for x, ok in zip(v.tolist(), RV.printable(v).tolist())]
    want += [repr(x / 1e4).encode() for x in d.tolist()]
    want += [str(np.round(np.float64(x), 2)).encode() if 0.0 <= x <= 1.0 else None for x in p.tolist()]
    values = list(v) + list(d) + list(p)
    for shift in range(8):
        check_items(dev, dev.rowtext_probe(values=v, fixed=d, prob=p, shift=shift), want, shift, values, 'mixed')
