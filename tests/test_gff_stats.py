"""The arithmetic of make_bed --gff --vo on the device (mcaller_amd/csrc/mc_npsum.h), host build: NumPy's order of additions restated
(tests/gffstats_files.py) equals NumPy bit for bit, the header equals the restatement, the printed text equals str() of NumPy's values,
and the random files of tests/test_gpu_bed_gff.py meet no decline.  No GPU."""
import struct
import warnings

import numpy as np
import pytest

from tests import gffstats_files as F


def bits(x):
    """The eight bytes of a double; every NaN is one value (0 / 0 has either sign, and both print as "nan")."""
    return b'nan' if x != x else struct.pack('<d', float(x))


def numpy_moments(p):
    a = np.array(p, dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return np.mean(a), np.var(a, ddof=1), np.std(a, ddof=1) / np.sqrt(len(a))


def arrays():
    out = [(n, F.seeded_array(n)) for n in F.N_LIST]
    return out + [(n, F.equal_array(n, v)) for n in (2, 9, 129) for v in (0.5, 0.62)] + [(3, [-0.5, 1e-9, 2.5e6]), (1, [0.0])]


@pytest.fixture(scope='module')
def cases():
    return [(n, p, numpy_moments(p)) for n, p in arrays()]


def test_the_restatement_is_numpys_summation(cases):
    for n, p, want in cases:
        got = F.moments(p)
        assert [bits(v) for v in got] == [bits(v) for v in want], (n, got, want)
    assert np.isnan(F.moments([0.3])[1]) and F.moments(F.equal_array(129))[2] == 0.0


def test_the_host_build_is_the_restatement(cases):
    from mcaller_amd import _lib
    for n, p, want in cases:
        st, mean, var, se = _lib.gff_site_moments(p)
        assert st == 0, (n, st)                                        # (8: the workgroup's tree is not the recursion)
        assert [bits(v) for v in (mean, var, se)] == [bits(v) for v in F.moments(p)], n
        for frac in (0.0, 1.0 / 3.0, 1.0):
            st, lo, up, qv = _lib.gff_site_stats(p, frac)
            se95 = 2 * want[2]
            assert st == (1 if n == 1 else 0)
            assert [bits(v) for v in (lo, up, qv)] == [bits(v) for v in (np.float64(frac) - se95, np.float64(frac) + se95, 100 * want[0])], n


def test_the_printed_text_is_str_of_numpys_values(cases):
    from mcaller_amd import _lib
    for n, p, want in cases:
        frac = np.float64(n // 2) / np.float64(n)
        se95 = 2 * want[2]
        text = ';fracLow=%s;fracUp=%s;identificationQv=%s' % (str(frac - se95), str(frac + se95), str(int(100 * want[0])))
        assert _lib.gff_site_text(p, frac) == text, n
    assert _lib.gff_site_text([0.3], 1.0) == ';fracLow=nan;fracUp=nan;identificationQv=30'
    assert _lib.gff_site_text([-0.004, -0.005], 0.0).endswith(';identificationQv=0')
    assert _lib.gff_site_text([-0.5, -0.75], 0.0).endswith(';identificationQv=-62')
    assert _lib.gff_site_text([1e20, 3e20], 0.5) is None and _lib.gff_site_stats([1e20, 3e20], 0.5)[0] & 4
    assert _lib.gff_site_stats([0.0, 4e9], 0.5)[0] == 2


def test_the_square_root_is_correctly_rounded():
    from mcaller_amd import _lib
    var, n = F.variances(20000)
    want = np.sqrt(np.array(var)) / np.sqrt(np.array(n))
    got = np.array([_lib.npsum_se(v, k) for v, k in zip(var, n)])
    assert (got == want).all()
    assert _lib.npsum_se(0.0, 4.0) == 0.0 and np.isnan(_lib.npsum_se(float('nan'), 1.0)) and _lib.npsum_se(5e-324, 1.0) == np.sqrt(5e-324)


def test_the_random_files_meet_no_decline(tmp_path):
    """Every written entry of the 300 random files: its probabilities are numbers mc_decimal.h reads as float() does, and the
    attribute text of the host build is make_bed's."""
    from mcaller_amd import _lib, make_bed
    n_entries = 0
    for seed in range(F.N_RANDOM):
        text, opts, _ = F.random_case(seed)
        src = tmp_path / 'r.diffs.6'
        src.write_bytes(text)
        rows = make_bed.read_diffs(str(src), None, keep_probs=True)
        for i in range(len(rows)):
            if not make_bed.selected(rows, i, None, opts['depth'], opts['thresh'], opts['control']):
                continue
            p = [_lib.parse_double(t) for t in rows.probs[i]]
            assert p == [float(t) for t in rows.probs[i]], (seed, rows.probs[i])
            with warnings.catch_warnings(), np.errstate(all='ignore'):
                warnings.simplefilter('ignore')
                want = make_bed.gff_attributes(rows, i, 'AMA', True)
            assert _lib.gff_site_text(p, rows.fraction(i)) == want[want.index(';fracLow='):], (seed, i)
            n_entries += 1
    assert n_entries > 1000
