"""Doubles, integers and probabilities for the row writer's number printing (mc_rowtext.h): the host build's test
(test_numerics.py) and the device's (test_gpu_rowtext_numbers.py) draw on the same sets."""
import math
import struct

import numpy as np

REPR_MIN, REPR_MAX = 1e-29, 1e9          # RT_REPR_MIN, RT_REPR_MAX


def printable(v):
    """Whether the row writer prints v (numpy array -> bool array): zero and RT_REPR_MIN <= |v| < RT_REPR_MAX; never nan or inf."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        a = np.abs(v)
        return (v == 0.0) | ((a >= REPR_MIN) & (a < REPR_MAX))


def shortest_values(rng):
    """Edge values, random mantissas over the whole range, slot means, read qualities, sums with a rounding residue, powers of two and
    ten with their neighbours, half-way cases and any bit pattern (a list of floats; rng: random.Random)."""
    vals = [-647985485.19140625, 2.9802322387695312e-08, 0.5, 0.25, 0.125, 1 / 3, 2 / 3, 7.055265349382997, 123456789.125, 5.551115123125783e-17,
            9.25185853854297e-18, 1.3552527156068805e-20]
    vals += [math.ldexp(1.0 + rng.random(), rng.randrange(-96, 29)) * rng.choice((-1, 1)) for _ in range(60000)]        # any mantissa, any exponent of the range
    vals += [rng.randrange(-2000000, 2000000) / (rng.randrange(1, 13) * 1e4) for _ in range(40000)]                      # slot means
    vals += [(rng.randrange(-2000000, 2000000) / 1e4) / rng.randrange(1, 13) for _ in range(40000)]
    vals += [round(rng.uniform(3, 40), rng.randrange(0, 16)) for _ in range(10000)]                                      # read qualities
    for _ in range(20000):                                                                                               # sums with a rounding residue
        n = rng.randrange(2, 10)
        xs = [rng.randrange(-100000, 100000) / 1e4 for _ in range(n)]
        vals.append((sum(xs) - sum(reversed(xs))) / n)
        vals.append(sum(xs) / n)
    for e in range(-96, 30):                                                                                            # powers of two (the lower gap is half the upper) ...
        p2 = math.ldexp(1.0, e)
        vals += [p2, float(np.nextafter(p2, 0.0)), float(np.nextafter(p2, 1e300))]
    for e in range(-29, 9):                                                                                             # ... and of ten, with their neighbours
        p10 = float('1e%d' % e)
        v = w = p10
        for _ in range(40):
            vals += [v, w]
            v, w = float(np.nextafter(v, 0.0)), float(np.nextafter(w, 1e300))
    vals += [(rng.getrandbits(rng.randrange(30, 54)) | 1) / math.ldexp(1.0, rng.randrange(1, 31)) for _ in range(40000)]    # short binary fractions: the half-way cases
    vals += [struct.unpack('<d', struct.pack('<Q', rng.getrandbits(64)))[0] for _ in range(20000)]                       # any bit pattern (mostly refused)
    return vals


def ulp_windows(centres, half=4096):
    """Every double within `half` ulps of each of `centres` (positive), the centres included: bit patterns counted up and down."""
    bits = np.asarray(centres, dtype=np.float64).view(np.int64)
    steps = np.arange(-half, half + 1, dtype=np.int64)
    return (bits[:, None] + steps[None, :]).reshape(-1).view(np.float64)


def branch_windows(half=4096):
    """+-half ulps around every power of two in [2^-96, 2^30) and every power of ten in [1e-29, 1e9]: where the decimal exponent's guess
    is put right, the gap below a power of two is half the one above, and the 64-bit / 128-bit switch moves."""
    p2 = [math.ldexp(1.0, e) for e in range(-96, 30)]
    p10 = [float('1e%d' % e) for e in range(-29, 10)]
    return ulp_windows(p2 + p10, half)


def slot_mean_values(rng, n_each=40000):
    """What slot means are, at scale (numpy generator rng): (d / 1e4) / n and (sum of n values d_i / 1e4) / n for n = 1..13, the sums
    made left to right in doubles; residues of sums that should be zero; means below 1e-3 (the 128-bit branch)."""
    out = []
    for n in range(1, 14):
        d = rng.integers(-2000000, 2000001, size=n_each)
        out.append((d / 1e4) / n)
        xs = rng.integers(-400000, 400001, size=(n_each, n)) / 1e4
        s = xs[:, 0].copy()
        for j in range(1, n):
            s += xs[:, j]
        out.append(s / n)
        # events and model means whose exact differences cancel: the residue of the sum in doubles
        a = rng.integers(-300000, 300001, size=(n_each // 4, n)) / 1e4
        r = a[:, 0].copy()
        for j in range(1, n):
            r += a[:, j]
        r -= a.sum(axis=1)
        out.append(r / n)
        small = rng.integers(-99, 100, size=n_each // 4) / 1e4            # |d| < 1e-2 over n: means below 1e-3
        out.append(small / n)
    fixed = [(0.1 + 0.2 - 0.3) / 3, (0.1 + 0.2 - 0.3) / 2, (0.0001 + 0.0 + 0.0) / 3, (0.3 - 0.1 - 0.2) / 5, 1.850371707708594e-17,
             3.3333333333333335e-05, (0.7 + 0.1 - 0.8) / 4, (1.1 + 2.2 - 3.3) / 3]
    out.append(np.array(fixed))
    # below 1e-3: any mantissa, every binary exponent down to the range's end
    m = 1.0 + rng.random(200000)
    e = rng.integers(-96, -9, size=200000)
    out.append(np.ldexp(m, e) * rng.choice((-1.0, 1.0), size=200000))
    return np.concatenate(out)


def layout_values(rng):
    """Every layout the row writer has and its 17th digit: 17-digit values, decimal exponents -28..9 (exponent form below -3),
    integers with trailing zeros, negatives, +-0."""
    out = [0.0, -0.0, 123456789.0, 1e8, 100000000.5, 120000.0, 10.0, 100.0, 1000.0, 1e4, 1e5, 1e6, 1e7, 9e8, 999999999.0,
           999999999.9999999, 123456789.125, 0.1 + 0.2, 1 / 3, 2 / 3, 1e-29, 1e-28, 1e-4, 1e-5, 0.001, 0.0001234, 12345678.9]
    out += [float('1e%d' % e) * k for e in range(-29, 9) for k in (1, 2, 5, 9)]
    for dp in range(-28, 10):                                                     # decpt: v in [10^(dp-1), 10^dp)
        lo = 10.0 ** (dp - 1)
        out += list(lo * (1.0 + 9.0 * rng.random(2000)))
        out += list(np.round(lo * (1.0 + 9.0 * rng.random(500)), max(0, 1 - dp)))    # few digits
    vals = np.array(out, dtype=np.float64)
    vals = vals[printable(vals)]
    return np.concatenate([vals, -vals])


def seventeen_digit_values(rng, n=50000):
    """Doubles whose repr has 17 significant digits (RtDigits.hi carries the first), over the whole range."""
    m = 1.0 + rng.random(n * 4)
    e = rng.integers(-96, 30, size=n * 4)
    v = np.ldexp(m, e)
    v = v[printable(v)]
    keep = [x for x in v.tolist() if len(repr(x).split('e')[0].replace('.', '').replace('-', '').lstrip('0')) == 17]
    return np.array(keep[:n], dtype=np.float64)


def digit_run_values(rng, n=100000):
    """A digit followed by 6 to 12 zeros or nines, then more digits: the remainder of the digit generation lands just above or just below
    a multiple of its divisor, where rt_small_quotient's float estimate of the next digit must be put right."""
    out = []
    for run in '09':
        lead = rng.integers(0, 10, size=(n // 2, 5))
        nlead = rng.integers(0, 6, size=n // 2)
        nrun = rng.integers(6, 13, size=n // 2)
        tail = rng.integers(0, 10, size=(n // 2, 6))
        ntail = rng.integers(1, 7, size=n // 2)
        first = rng.integers(1, 10, size=n // 2)
        exp = rng.integers(-28, 10, size=n // 2)
        for i in range(n // 2):
            m = (str(first[i]) + ''.join(map(str, lead[i, :nlead[i]])) + str(first[(i + 1) % (n // 2)]) + run * nrun[i] +
                 ''.join(map(str, tail[i, :ntail[i]])))[:17]
            out.append(float('0.%se%d' % (m, exp[i])))
    v = np.array(out, dtype=np.float64)
    return np.concatenate([v, -v[: n // 10]])


def random_patterns(rng, n=200000):
    """Any 64-bit pattern: nan, inf, subnormals, huge -- mostly refused."""
    return rng.integers(-2 ** 63, 2 ** 63 - 1, size=n, dtype=np.int64, endpoint=True).view(np.float64)


def fixed4_values(rng):
    """Integer slot means d (printed as repr(d / 1e4)): every d in [-2e6, 2e6], the ends of int32 and their neighbours, 10^6 random
    int32, every trailing-zero pattern."""
    ends = [-2 ** 31, -2 ** 31 + 1, -2 ** 31 + 2, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 3, -1, 0, 1]
    tz = [s * k * 10 ** z for z in range(0, 10) for k in (1, 2, 5, 7, 9, 11, 99, 123, 1001) for s in (1, -1) if k * 10 ** z < 2 ** 31]
    return np.concatenate([np.arange(-2000000, 2000001, dtype=np.int64), np.array(ends + tz, dtype=np.int64),
                           rng.integers(-2 ** 31, 2 ** 31, size=1000000, dtype=np.int64)]).astype(np.int32)


def prob_values(rng):
    """Probabilities (printed as np.round(p, 2)): j / 200 with +-1, +-2 ulps, 0, 1, the double below 1, values whose p * 100 lands
    on .5, and 10^6 uniform values."""
    grid = np.arange(201) / 200.0
    near = [grid]
    up, down = grid.copy(), grid.copy()
    for _ in range(2):
        up, down = np.nextafter(up, 2.0), np.nextafter(down, -1.0)
        near += [up, down]
    edge = np.array([0.0, 1.0, float(np.nextafter(1.0, 0.0)), 0.285, 0.145, 0.005, 0.015, 0.995, 0.125, 0.375, 0.5, 0.625, 0.875,
                     5e-324, 1e-300, 0.004999999999999999, 0.0050000000000000001])
    halves = (np.arange(100) + 0.5) / 100.0                                  # p * 100 near k + 0.5
    p = np.concatenate(near + [edge, halves, np.nextafter(halves, 0.0), np.nextafter(halves, 1.0), rng.random(1000000)])
    return p[(p >= 0.0) & (p <= 1.0)]
