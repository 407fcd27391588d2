#!/usr/bin/env python3
"""tools/hypergeom_error.py [--device] [--masses] [--json profiles/hypergeom_error.json]

The error of mc_hypergeom.h's tail P(X >= k), X ~ Hypergeometric(N, K, d), against exact rationals: the largest
|tail - exact| and the largest DERIVED bound `err` the header returns beside it, over

    N in SIZES (1 .. 2000, sampled), every K in 0 .. N, d in {1, 2, 5, 15, 50, 256, 1024} with d <= N, every k in 0 .. d + 1.

The host build (mc_hypergeom_tail_many) is measured on any machine; --device measures the device build too
(mc_hypergeom_tail_device, a launch per (N, d)) and needs a GPU.  A case whose error exceeds its bound is a violation: the
derivation in the header is wrong then, and the tool exits with 1.  scipy.stats.hypergeom.sf is held against the same tails
for N <= 300 as a cross-check of the exact side (its own error is not known; the figure is on record, nothing depends on it).

--masses measures hg_masses instead (mc_hypergeom_masses_many; with --device mc_hypergeom_masses_device too), on the same N, K and
d: the sum over the 101 buckets of |mass - exact| against the ONE derived bound a (N, K, d) gets, which bounds every tail formed
from the masses.  It writes the record's `masses` section and leaves the rest as it is.

The record keeps a `device` entry it already has when it is run without --device."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import hypergeom_grid as G  # noqa: E402  (the exact side: integers only)

SIZES = list(range(1, 13)) + [15, 20, 30, 50, 64, 100, 150, 256, 300, 500, 700, 1000, 1024, 1025, 1500, 2000]
DEPTHS = (1, 2, 5, 15, 50, 256, 1024)


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


class Figures(object):
    def __init__(self):
        self.cases, self.violations, self.measured_max, self.err_max, self.at, self.per_d = 0, 0, 0.0, 0.0, None, {}

    def take(self, N, d, Ks, ks, tail, err, exact):
        """exact[i] = (num list, den) of case i's (N, K, d)."""
        self.cases += len(tail)
        self.err_max = max(self.err_max, float(err.max()))
        worst = self.per_d.get(str(d), 0.0)
        for i in range(len(tail)):
            num, den = exact[i]
            n = num[ks[i]]
            if err[i] == 0.0:                                  # a trivial case: exact, or a violation
                if not ((tail[i] == 1.0 and n == den) or (tail[i] == 0.0 and n == 0)):
                    self.violations += 1
                continue
            e = G.abs_error(tail[i], n, den)
            if e > 0.5 * err[i] and not G.within(tail[i], err[i], n, den):
                self.violations += 1
            if e > self.measured_max:
                self.measured_max, self.at = e, dict(N=int(N), K=int(Ks[i]), d=int(d), k=int(ks[i]))
            worst = max(worst, e)
        self.per_d[str(d)] = worst

    def record(self):
        return dict(cases=self.cases, violations=self.violations, measured_max=self.measured_max, at=self.at,
                    derived_err_max=self.err_max, margin=self.err_max / self.measured_max if self.measured_max else None, per_d=self.per_d)


class MassFigures(object):
    SHIFT = 1100                                              # every mass is a multiple of 2^-1100 (a double of 2^-1022 or more, 53 bits)

    def __init__(self):
        self.cases, self.violations, self.measured_max, self.err_max, self.at = 0, 0, 0.0, 0.0, None

    def take(self, N, d, mass, err, per_K):
        """mass[K], err[K] of (N, K, d) for every K; per_K[K] = (num list, den)."""
        one = 1 << self.SHIFT
        first = [0] * 103                                     # bucket c holds the x of first[c] .. first[c + 1] - 1
        for c in range(1, 103):
            first[c] = min(d + 1, -(-(c - 1) * d // 100))     # the least x with 100 x >= (c - 1) d
        for K in range(N + 1):
            num, den = per_K[K]
            total = 0
            for c in range(1, 102):
                ta, tb = float(mass[K][c]).as_integer_ratio()
                total += abs(ta * (one // tb) * den - (num[first[c]] - num[first[c + 1]]) * one)
            self.cases += 1
            e = float(err[K])
            self.err_max = max(self.err_max, e)
            ea, eb = e.as_integer_ratio()
            if not (mass[K][0] == 0.0 and total * eb <= ea * den * one):
                self.violations += 1
            measured = total / (den * one)
            if measured > self.measured_max:
                self.measured_max, self.at = measured, dict(N=int(N), K=int(K), d=int(d))

    def record(self):
        return dict(cases=self.cases, violations=self.violations, measured_max=self.measured_max, at=self.at,
                    derived_err_max=self.err_max, margin=self.err_max / self.measured_max if self.measured_max else None)


def main_masses(path, device):
    from mcaller_amd import _lib
    host, dev = MassFigures(), MassFigures()
    t0 = time.time()
    for N in SIZES:
        for d in DEPTHS:
            if d > N:
                continue
            per_K = [G.tail_numerators(N, K, d) for K in range(N + 1)]
            Ks = np.arange(N + 1, dtype=np.int64)
            Ns, ds = np.full(N + 1, N, dtype=np.int64), np.full(N + 1, d, dtype=np.int64)
            host.take(N, d, *_lib.hypergeom_masses(Ns, Ks, ds), per_K)
            if device is not None:
                dev.take(N, d, *device.hypergeom_masses(Ns, Ks, ds), per_K)
        print('N = %d done, %.0f s' % (N, time.time() - t0), file=sys.stderr)
    rec = json.load(open(path)) if os.path.exists(path) else {}
    old = rec.get('masses') or {}
    rec['masses'] = {
        'what': 'sum over the buckets c = 1 .. 101 of |mass[c] - exact| of hg_masses (mcaller_amd/csrc/mc_hypergeom.h) against exact '
                'rationals; derived_err_max is the largest bound the header returned; one case is one (N, K, d)',
        'grid': 'N in %s; every K in 0 .. N; d in %s with d <= N' % (SIZES, list(DEPTHS)),
        'host': host.record(),
        'device': dev.record() if device is not None else old.get('device'),
    }
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec['masses']))
    return 1 if host.violations or dev.violations else 0


def main():
    from mcaller_amd import _lib
    path = arg('--json', os.path.join(REPO, 'profiles', 'hypergeom_error.json'))
    device = None
    if '--device' in sys.argv:
        from mcaller_amd.device import get_device
        device = get_device()
    if '--masses' in sys.argv:
        return main_masses(path, device)
    host, dev = Figures(), Figures()
    scipy_diff, scipy_version = 0.0, None
    try:
        import scipy
        from scipy import stats
        scipy_version = scipy.__version__
    except ImportError:
        stats = None
    t0 = time.time()
    for N in SIZES:
        for d in DEPTHS:
            if d > N:
                continue
            per_K = [G.tail_numerators(N, K, d) for K in range(N + 1)]
            Ks = np.repeat(np.arange(N + 1, dtype=np.int64), d + 2)
            ks = np.tile(np.arange(d + 2, dtype=np.int64), N + 1)
            Ns, ds = np.full(len(Ks), N, dtype=np.int64), np.full(len(Ks), d, dtype=np.int64)
            exact = [per_K[K] for K in Ks]
            tail, err = _lib.hypergeom_tail(Ns, Ks, ds, ks)
            host.take(N, d, Ks, ks, tail, err, exact)
            if device is not None:
                dt, de = device.hypergeom_tail(Ns, Ks, ds, ks)
                dev.take(N, d, Ks, ks, dt, de, exact)
            if stats is not None and N <= 300:
                scipy_diff = max(scipy_diff, float(np.abs(stats.hypergeom.sf(ks - 1, N, Ks, d) - tail).max()))
        print('N = %d done, %.0f s' % (N, time.time() - t0), file=sys.stderr)
    old = json.load(open(path)) if os.path.exists(path) else {}
    rec = {
        'masses': old.get('masses'),
        'what': '|tail - exact| of P(X >= k), X ~ Hypergeometric(N, K, d), by mcaller_amd/csrc/mc_hypergeom.h against exact rationals; '
                'derived_err_max is the largest bound the header returned on the grid',
        'grid': 'N in %s; every K in 0 .. N; d in %s with d <= N; every k in 0 .. d + 1' % (SIZES, list(DEPTHS)),
        'numpy': np.__version__,
        'host': host.record(),
        'device': dev.record() if device is not None else old.get('device'),
        'scipy': scipy_version,
        'scipy_sf_max_abs_diff_n_le_300': scipy_diff if stats is not None else None,
        'scipy_sf_within_derived_bound': (scipy_diff <= host.err_max) if stats is not None else None,
    }
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps({k: rec[k] for k in ('host', 'device', 'scipy_sf_max_abs_diff_n_le_300')}))
    return 1 if host.violations or dev.violations else 0


if __name__ == '__main__':
    sys.exit(main())
