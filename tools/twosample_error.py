#!/usr/bin/env python3
"""tools/twosample_error.py -- measure the two tail functions of mcaller_amd/csrc/mc_twosample.h (host build) against SciPy over the
grid of tests/twosample_grid.py and write profiles/twosample_error.json: the figures TW_FN_BOUND is made from (the largest x 64,
rounded up).  No GPU needed."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import numpy
    import scipy
    from tests import twosample_grid as G
    m = G.measure()
    largest = max(m['normal']['max_vs_sf'], m['normal']['max_vs_logsf'], m['kolmogorov']['max'])
    doc = {
        'what': '|mc_twosample.h log10 p - SciPy log10 p| / max(1, |log10 p|), host build: tw_log10_2sf against log10(2 * norm.sf(z)) and '
                '(log 2 + norm.logsf(z)) / log 10, tw_log10_kolmogorov against log10(scipy.special.kolmogorov(lambda))',
        'grid': 'tests/twosample_grid.py: z 1e-6 .. 40 and lambda 1e-6 .. 20, evenly in log and evenly, cut where log10 p < -290',
        'scipy': scipy.__version__, 'numpy': numpy.__version__,
        'normal': m['normal'], 'kolmogorov': m['kolmogorov'],
        'measured_max': largest, 'times_64': largest * 64, 'bound': G.FN_BOUND, 'margin': G.FN_BOUND / largest,
    }
    path = os.path.join(REPO, 'profiles', 'twosample_error.json')
    with open(path, 'w') as fo:
        json.dump(doc, fo, indent=1)
        fo.write('\n')
    print(json.dumps(doc, indent=1))


if __name__ == '__main__':
    main()
