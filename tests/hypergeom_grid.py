"""The small grid mc_hypergeom.h's two builds are held against exact rationals on (tests/test_hypergeom.py the host build,
tests/test_gpu_hypergeom.py the device build, one launch), and the exact side itself: integers only, no gcd.

tools/hypergeom_error.py measures on a far larger grid (profiles/hypergeom_error.json); this one keeps every path of hg_tail --
the trivial ends, both walks, a walk that stops below 2^-900, d = N, K = 0 and K = N -- at a size a test can afford."""
import math

import numpy as np

DEPTHS = (1, 2, 5, 15, 50, 256, 1024)
SIZES = (1, 2, 3, 5, 8, 13, 30, 64, 100, 257, 600, 1500, 2000)


def tail_numerators(N, K, d):
    """-> (num[0 .. d + 1], den): P(X >= x) = num[x] / den for X ~ Hypergeometric(N, K, d); num[d + 1] = 0."""
    lo, hi = max(0, d - (N - K)), min(K, d)
    term = [0] * (d + 2)                                  # C(K, x) C(N - K, d - x): two binomials at lo, then the exact integer ratio
    term[lo] = math.comb(K, lo) * math.comb(N - K, d - lo)
    for x in range(lo, hi):
        term[x + 1] = term[x] * ((K - x) * (d - x)) // ((x + 1) * (N - K - d + x + 1))
    num = [0] * (d + 2)
    for x in range(d, -1, -1):
        num[x] = num[x + 1] + term[x]
    den = math.comb(N, d)
    assert num[0] == den                                  # Vandermonde: the terms are the whole of C(N, d)
    return num, den


def abs_error(tail, num, den):
    """|tail - num / den| as a float, correctly rounded (Python's integer quotient)."""
    ta, tb = float(tail).as_integer_ratio()
    return abs(ta * den - num * tb) / (tb * den)


def within(tail, err, num, den):
    """|tail - num / den| <= err, decided in integers."""
    if not (err >= 0.0 and err < float('inf')):
        return False
    ta, tb = float(tail).as_integer_ratio()
    ea, eb = float(err).as_integer_ratio()
    return abs(ta * den - num * tb) * eb <= ea * tb * den


def _some(n, every_below):
    """0 .. n: all of them up to `every_below`, else the ends, the thirds and their neighbours."""
    if n <= every_below:
        return list(range(n + 1))
    picks = {0, 1, 2, n - 2, n - 1, n}
    for q in (n // 3, n // 2, (2 * n) // 3, (9 * n) // 10):
        picks |= {q - 1, q, q + 1}
    return sorted(p for p in picks if 0 <= p <= n)


_cases = None


def cases():
    """-> (N, K, d, k int64 arrays, [(num, den)] per case).  k runs from -1 to d + 2 where it runs over everything."""
    global _cases
    if _cases is None:
        N_, K_, d_, k_, exact = [], [], [], [], []
        for N in SIZES:
            for d in DEPTHS + (N,):
                if d > N:
                    continue
                for K in _some(N, 30):
                    num, den = tail_numerators(N, K, d)
                    ks = [-1] + (list(range(d + 2)) if d <= 50 else _some(d + 1, 0) + _some(min(K, d) + 1, 0)) + [d + 2]
                    # around the mode, where both walks run
                    mode = ((d + 1) * (K + 1)) // (N + 2)
                    ks += [x for x in (mode - 1, mode, mode + 1) if 0 <= x <= d + 1]
                    for k in sorted(set(ks)):
                        N_.append(N); K_.append(K); d_.append(d); k_.append(k)
                        exact.append((den if k < 0 else 0 if k > d + 1 else num[k], den))
        _cases = tuple(np.asarray(a, dtype=np.int64) for a in (N_, K_, d_, k_)) + (exact,)
    return _cases
