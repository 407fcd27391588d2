"""The grid the errors of mc_twosample.h's two tail functions are measured on (profiles/twosample_error.json, written by
tools/twosample_error.py; tests/test_twosample.py): |z| and lambda from 1e-6 up to where log10 p reaches -290, with SciPy's value of
log10 p beside every point."""
import numpy as np

FN_BOUND = 8.0e-14                 # TW_FN_BOUND of mc_twosample.h: relative to max(1, |log10 p|)
LOG10P_MIN = -290.0


def normal_grid():
    """-> (z [k], log10(2 norm.sf(z)) [k], (log 2 + norm.logsf(z)) / log 10 [k]): 400 z spaced evenly in log from 1e-6 to 40 and 800
    spaced evenly from 0.01 to 40, cut where log10 p falls below -290."""
    from scipy.stats import norm
    z = np.concatenate([np.logspace(-6, np.log10(40.0), 400), np.linspace(0.01, 40.0, 800)])
    with np.errstate(all='ignore'):
        by_sf = np.log10(2 * norm.sf(z))
        by_logsf = (np.log(2.0) + norm.logsf(z)) / np.log(10.0)
    keep = np.isfinite(by_sf) & (by_sf >= LOG10P_MIN)
    return z[keep], by_sf[keep], by_logsf[keep]


def kolmogorov_grid():
    """-> (lambda [k], log10(scipy.special.kolmogorov(lambda)) [k]): 400 lambda spaced evenly in log from 1e-6 to 20 and 800 spaced
    evenly from 0.01 to 20 (both forms of the series and the change between them at 1), cut where log10 p falls below -290."""
    from scipy import special
    lam = np.concatenate([np.logspace(-6, np.log10(20.0), 400), np.linspace(0.01, 20.0, 800), [0.999999, 1.0, 1.000001]])
    with np.errstate(all='ignore'):
        l = np.log10(special.kolmogorov(lam))
    keep = np.isfinite(l) & (l >= LOG10P_MIN)
    return lam[keep], l[keep]


def relative_error(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def measure():
    """The largest relative error of the host build of each tail function over its grid -> dict (what the profile records)."""
    from mcaller_amd import _lib
    z, by_sf, by_logsf = normal_grid()
    got = np.asarray([_lib.twosample_log10_2sf(v) for v in z])
    e_sf, e_logsf = relative_error(got, by_sf), relative_error(got, by_logsf)
    lam, want = kolmogorov_grid()
    got_k = np.asarray([_lib.twosample_log10_kolmogorov(v) for v in lam])
    e_k = relative_error(got_k, want)
    return dict(normal=dict(points=int(len(z)), max_vs_sf=float(e_sf.max()), at_vs_sf=float(z[e_sf.argmax()]),
                            max_vs_logsf=float(e_logsf.max()), at_vs_logsf=float(z[e_logsf.argmax()]), z_max=float(z.max())),
                kolmogorov=dict(points=int(len(lam)), max=float(e_k.max()), at=float(lam[e_k.argmax()]), lambda_max=float(lam.max())))
