#!/usr/bin/env python3
"""tools/fisher_error.py [--device] [--json profiles/fisher_error.json]

The error of mc_fisher.h's log10 p of Fisher's exact test against exact rationals: the largest |log10 p - exact| and the largest
DERIVED bound the header returns beside it, over the grid of tests/fisher_bh_cases.py:

    every table with 1 <= n1, n2 <= 12 (8100), and the seeded tables with pooled sizes up to 8192 (random, lo > 0, K = 0, K = N,
    mirrored symmetric pairs, the deepest sites, tables beyond the far tail).

`exact` is the fp64 number nearest to log10 of the rational p (mpmath, 60 digits).  The host build (mc_fisher_exact_many) is
measured on any machine; --device measures the device build too (mc_fisher_exact_device, a lane per table) and needs a GPU, and
says whether the two builds' bits are equal.  A case above its bound is a violation: the derivation in the header is wrong then, and
the tool exits with 1.  The host statement (compare_genomes.fisher_log10p) is held against scipy.stats.fisher_exact on 3000 seeded
tables with n < 80, and bh_log10 against scipy.stats.false_discovery_control on 1000 seeded p: both figures are on record.
The record keeps a `device` entry it already has when it is run without --device."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import fisher_bh_cases as F  # noqa: E402  (the exact side)


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def measure(L, bound, status, exact):
    ok = np.isfinite(bound)
    err = np.abs(L[ok] - exact[ok])
    return dict(cases=int(len(L)), vouched=int(ok.sum()), far_tail=int(np.count_nonzero(status & 2)), select=int(np.count_nonzero(status & 4)),
                largest_error=float(err.max()), largest_bound=float(bound[ok].max()), violations=int(np.count_nonzero(err > bound[ok])),
                largest_error_over_bound=float(np.max(err[bound[ok] > 0] / bound[ok][bound[ok] > 0])))


def main():
    from mcaller_amd import _lib, compare_genomes as CG
    out = arg('--json', os.path.join(REPO, 'profiles', 'fisher_error.json'))
    t0 = time.time()
    small, deep = F.small_tables(), [c[1:] for c in F.seeded_tables()]
    tables = small + deep
    exact = np.asarray([F.log10_exact(F.fisher_p(*t)[0]) for t in small] + [F.log10_exact(F.fisher_p(*t, walked=True)[0]) for t in deep])
    K1, n1, K2, n2 = np.asarray(tables, dtype=np.int64).T
    hl, hb, hs = _lib.fisher_exact(K1, n1, K2, n2)
    record = dict(tool='tools/fisher_error.py', grid='every table with n1, n2 <= 12; tests/fisher_bh_cases.seeded_tables (pooled sizes up to 8192)',
                  host=measure(hl, hb, hs, exact))
    if os.path.exists(out):
        old = json.load(open(out))
        if 'device' in old:
            record['device'] = old['device']
    if '--device' in sys.argv:
        from mcaller_amd.device import get_device
        dl, db, ds = get_device().fisher_exact(K1, n1, K2, n2)
        record['device'] = dict(measure(dl, db, ds, exact), status_equal=bool(np.array_equal(hs, ds)),
                                bits_equal=bool(np.array_equal(hl, dl) and np.array_equal(hb, db)),
                                largest_host_device_difference=float(np.max(np.abs(hl[np.isfinite(hb)] - dl[np.isfinite(hb)]))))
    from scipy.stats import false_discovery_control, fisher_exact
    rng = np.random.default_rng(53)
    worst = 0.0
    for _ in range(3000):
        a, b = (int(v) for v in rng.integers(1, 80, size=2))
        k1, k2 = int(rng.integers(0, a + 1)), int(rng.integers(0, b + 1))
        p = float(F.fisher_p(k1, a, k2, b)[0])
        worst = max(worst, abs(p - fisher_exact([[k1, a - k1], [k2, b - k2]])[1]) / p)
    p = np.random.default_rng(59).random(1000) ** 2
    fdc = false_discovery_control(p)
    record['host_statement'] = dict(fisher_relative_difference_to_scipy=worst, tables=3000,
                                    bh_relative_difference_to_false_discovery_control=float(np.max(np.abs(10.0 ** CG.bh_log10(np.log10(p)) - fdc) / fdc)))
    record['seconds'] = round(time.time() - t0, 1)
    with open(out, 'w') as fh:
        json.dump(record, fh, indent=1)
        fh.write('\n')
    print(json.dumps(record))
    bad = record['host']['violations'] + record.get('device', {}).get('violations', 0)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
