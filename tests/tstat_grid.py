"""The grid the error of mc_tstat.h's tail function is measured on (profiles/tstat_error.json; tests/test_tstat.py,
tests/test_gpu_bed_positions.py): degrees of freedom 1 .. 10^5 x |t| from 10^-6 up to where log10 p reaches -290, with SciPy's
value of log10 p beside every point."""
import numpy as np

DFS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 15, 20, 31, 32, 33, 50, 64, 100, 256, 257, 1000, 4999, 10000, 31623, 100000]
FN_BOUND = 4.0e-13                 # TS_FN_BOUND of mc_tstat.h: relative to max(1, |log10 p|)
LOG10P_MIN = -290.0


def grid():
    """-> (df [k], t [k], SciPy's log10 p [k]); every df with 600 |t| spaced evenly in log from 1e-6 to 1e300 and 200 spaced
    evenly from 0.05 to 45 (where a large df has its whole range), cut where log10 p falls below -290."""
    from scipy import special
    dfs, ts, ls = [], [], []
    for df in DFS:
        t = np.concatenate([np.logspace(-6, 300, 600), np.linspace(0.05, 45.0, 200)])
        with np.errstate(all='ignore'):
            l = np.log10(2 * special.stdtr(df, -t))
        keep = np.isfinite(l) & (l >= LOG10P_MIN)
        dfs.append(np.full(keep.sum(), float(df))); ts.append(t[keep]); ls.append(l[keep])
    return np.concatenate(dfs), np.concatenate(ts), np.concatenate(ls)


def triples(df, t):
    """(n, mean, var) whose statistic is t with df degrees of freedom: n = df + 1, var = n, so that t = mean exactly."""
    n = df + 1.0
    return n, t.copy(), n.copy()


def relative_error(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))
