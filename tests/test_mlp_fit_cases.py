"""The case table of tests/mlp_fit_cases.py against the oracle alone (no GPU): every case reaches the edge it names, and keeps the
margins that let tests/test_gpu_mlp_fit_shapes.py ask for EQUAL epoch counts and held-out counts.  These are conditions on the inputs
(seeds are picked to keep them), not measurements of the device."""
import numpy as np
import pytest

from oracle import mlp_fit_oracle as mo
from tests import mlp_fit_cases as MC

ALL = dict(MC.CASES, **{MC.WORKER_CASE['name']: MC.WORKER_CASE})


def by_edge(edge):
    return sorted(n for n, c in MC.CASES.items() if c['edge'] == edge)


def batches_of(n, batch_size):
    """Sizes of an epoch's batches as mo.fit and the kernel cut them."""
    b = min(batch_size, n)
    return [min(b, n - b0) for b0 in range(0, n, b)]


def test_the_table_holds_what_the_gaps_ask_for():
    names = set(MC.CASES)
    for h in (1, 2, 63, 64, 65, 100, 127, 128):
        four, one = MC.CASES['width_%d_four_wgs' % h], MC.CASES['width_%d_one_wg' % h]
        assert (four['hidden'], four['d'], four['batch_size'], four['n']) == (h, 7, 64, 150)
        assert (one['hidden'], one['d'], one['batch_size'], one['n']) == (h, 7, 32, 80)
    for d in (1, 2, 8, 9):
        for path in ('four_wgs', 'one_wg'):
            c = MC.CASES['inputs_%d_%s' % (d, path)]
            assert (c['d'], c['hidden']) == (d, 65) and MC.problem(c)[0].shape[1] == d
    assert {'last_batch_%d_four_wgs' % r for r in (1, 2, 15, 16, 17, 31, 32, 33, 63)} <= names
    assert {'last_batch_%d_one_wg' % r for r in (1, 3, 4, 5, 7, 8, 9, 15)} <= names
    assert {'rows_%d_%s' % (n, p) for n in (1, 2, 3) for p in ('four_wgs', 'one_wg')} | {'rows_63_batch_200'} <= names
    assert [MC.CASES['batch_%d' % b]['batch_size'] for b in (63, 64, 255, 256)] == [63, 64, 255, 256]
    assert (MC.CASES['batch_63']['n'], MC.CASES['batch_64']['n']) == (200, 200)
    for b in (255, 256):
        c = MC.CASES['batch_%d' % b]
        assert (c['n'], c['d'], c['hidden']) == (600, 9, 128)
    assert [MC.CASES['perm_%d' % n]['batch_size'] for n in (16, 17, 64, 65, 256, 257, 1024, 1025)] == [4, 4, 16, 16, 64, 64, 200, 200]
    for name in by_edge('stop'):
        c = MC.CASES[name]
        assert (c['hidden'], c['tol'], c['n_iter_no_change'], len(c['seeds'])) == (16, 1e-2, 2, 6)
    assert (MC.CASES['stop_batch_200']['max_iter'], MC.CASES['stop_batch_32']['max_iter']) == (60, 25)
    assert len(by_edge('clip')) == 4 and all(MC.CASES[n]['max_iter'] == 8 and MC.CASES[n]['hidden'] == 100 for n in by_edge('clip'))
    w = MC.WORKER_CASE
    assert (len(w['seeds']), w['hidden'], w['batch_size'], w['n'], w['max_iter']) == (6, 100, 200, 450, 12)
    for c in ALL.values():                       # every job its own seed; both classes wherever there are two rows
        assert len(set(c['seeds'])) == len(c['seeds']) and c['shuffle'] and 8 <= c['max_iter'] <= 60 and c['n'] <= 1100
        X, y = MC.problem(c)
        assert X.shape == (c['n'] + MC.N_VAL, c['d']) and X.dtype == np.float64 and y.dtype == np.uint8
        if c['n'] >= 2:
            assert set(y[:c['n']].tolist()) == {0, 1}, c['name']


@pytest.mark.parametrize('name', sorted(n for n, c in MC.CASES.items() if 'wgs' in c['expect']))
def test_case_takes_the_path_it_names(name):
    c = MC.CASES[name]
    assert MC.workgroups(c['batch_size']) == c['expect']['wgs']
    assert ('four_wgs' in name) <= (c['expect']['wgs'] == 4) and ('one_wg' in name) <= (c['expect']['wgs'] == 1)


@pytest.mark.parametrize('name', sorted(n for n, c in MC.CASES.items() if 'last_batch' in c['expect']))
def test_last_batch_is_the_size_named(name):
    c = MC.CASES[name]
    for tr, _ in MC.job_rows(c):
        sizes = batches_of(len(tr), c['batch_size'])
        assert sizes[-1] == c['expect']['last_batch'] and len(sizes) == c['expect']['batches']
    if c['edge'] == 'last_batch':                # ... and sits where the name says, relative to the waves that share a batch
        gw = MC.WAVES * c['expect']['wgs']
        assert c['expect']['last_batch'] in (1, 2, 3, gw - 1, gw, gw + 1, 2 * gw - 1, 2 * gw, 2 * gw + 1, c['batch_size'] - 1)


def test_last_batches_cover_both_sides_of_the_wave_count():
    for path, gw in (('four_wgs', 16), ('one_wg', 4)):
        have = {MC.CASES[n]['expect']['last_batch'] for n in by_edge('last_batch') if n.endswith(path)}
        assert {gw - 1, gw, gw + 1, 2 * gw - 1, 2 * gw, 2 * gw + 1} <= have


@pytest.mark.parametrize('name', by_edge('perm'))
def test_permutation_size_is_on_the_side_named(name):
    c = MC.CASES[name]
    n, want = c['n'], c['expect']
    assert MC.perm_bits(n) == want['bits'] and len(batches_of(n, c['batch_size'])) >= want['min_batches']
    assert ((1 << want['bits']) == n) == (not want['walks'])
    assert len(c['seeds']) == 2
    orders = [mo.epoch_order(n, s, e) for s in c['seeds'] for e in (0, 1)]
    for o in orders:
        assert sorted(o.tolist()) == list(range(n)) and (o != np.arange(n)).any()
    assert (orders[0] != orders[1]).any() and (orders[0] != orders[2]).any()
    if want['walks']:                            # some index leaves the range on its first round trip and is walked on
        half, mask = want['bits'] // 2, (1 << (want['bits'] // 2)) - 1
        key = mo.epoch_key(c['seeds'][0], 0)

        def once(x):
            L, R = x >> half, x & mask
            for r in range(4):
                L, R = R, L ^ (mo._mix32(R * 0x9E3779B1 + key + r * 0x85EBCA6B) & mask)
            return (L << half) | R
        assert any(once(i) >= n for i in range(n))


def test_permutation_cases_sit_on_both_sides_of_each_even_power():
    bits = {c['n']: c['expect']['bits'] for c in MC.CASES.values() if c['edge'] == 'perm'}
    assert bits == {16: 4, 17: 6, 64: 6, 65: 8, 256: 8, 257: 10, 1024: 10, 1025: 12}


@pytest.mark.parametrize('name', by_edge('stop'))
def test_stopping_jobs_stop_apart_and_never_on_the_line(name):
    """At every epoch of every job the oracle's loss stays 1e-5 (ten times the device tests' loss tolerance at these magnitudes) away
    from best - tol, so the device cannot legitimately decide an epoch differently; the jobs leave the loop at different epochs and
    one of them later than all the others."""
    c = MC.CASES[name]
    fits = MC.oracle(c)
    stops = [f['n_iter'] for f in fits]
    assert len(set(stops)) >= 2 and sorted(stops)[-1] > sorted(stops)[-2], stops
    assert max(stops) <= 25 and min(stops) < c['max_iter'], stops
    for f in fits:
        best, no_improve = np.inf, 0
        for loss in f['loss_curve']:
            assert abs(loss - (best - c['tol'])) >= 1e-5
            no_improve = no_improve + 1 if loss > best - c['tol'] else 0
            best = min(best, loss)
        assert (no_improve > c['n_iter_no_change']) == (f['n_iter'] < c['max_iter'])
    for tr, _ in MC.job_rows(c):
        assert len(batches_of(len(tr), c['batch_size'])) >= 2      # the order of the rows matters


@pytest.mark.parametrize('name', by_edge('clip'))
def test_clip_cases_pass_700_on_both_classes(name):
    c = MC.CASES[name]
    X, y = MC.problem(c)
    X, y = X[:c['n']], y[:c['n']]
    [start], [fit] = MC.start_weights(c), MC.oracle(c)
    assert (start[2] == (8.0 if '+8' in name else -8.0)).all() and c['x_scale'] == 30.0
    for W1, b1, W2, b2 in (start, (fit['W1'], fit['b1'], fit['W2'], fit['b2'])):
        out = np.tanh(X @ W1 + b1) @ W2 + b2
        with np.errstate(over='ignore'):
            p = 1.0 / (1.0 + np.exp(-out))
        for label in (0, 1):
            assert ((out > 700) & (y == label)).sum() >= 1 and ((out < -700) & (y == label)).sum() >= 1
            assert ((p == 0.0) & (y == label)).sum() >= 1 and ((p == 1.0) & (y == label)).sum() >= 1
        assert (out < -709.8).any()              # exp(-out) overflows
    # the clip decides the loss: a row on the wrong side costs -log(eps) = 36.04, without the clip the loss would be infinite
    wrong = -np.log(np.finfo(np.float64).eps)
    assert np.isfinite(fit['loss_curve']).all() and fit['loss_curve'][0] > wrong / c['n']
    assert fit['n_iter'] == 8


@pytest.mark.parametrize('name', by_edge('jobs') + by_edge('empty'))
def test_job_counts(name):
    c = MC.CASES[name]
    jobs = MC.job_rows(c)
    if c['edge'] == 'jobs':
        assert len(jobs) == int(name.split('_')[1]) and name in ('jobs_8', 'jobs_9')
        assert tuple(sorted({len(va) for _, va in jobs})) == c['expect']['fold_sizes']
        assert c['expect']['fold_sizes'][1] - c['expect']['fold_sizes'][0] == 1
        for tr, va in jobs:
            assert len(tr) + len(va) == c['n'] and not set(tr.tolist()) & set(va.tolist())
    else:
        assert [len(tr) > 0 for tr, _ in jobs] == [True, False, True] and all(len(va) > 0 for _, va in jobs)
        mid = MC.oracle(c)[1]
        W1, b1, W2, b2 = mo.init_weights(c['d'], c['hidden'], c['seeds'][1])
        assert mid['n_iter'] == 0 and len(mid['loss_curve']) == 0
        assert (mid['W1'] == W1).all() and (mid['b1'] == b1).all() and (mid['W2'] == W2).all() and mid['b2'] == b2
        X, y = MC.problem(c)
        va = jobs[1][1]
        assert mid['val_correct'] == int(((mo.forward(W1, b1, W2, b2, X[va])[1] > 0.5) == (y[va] > 0)).sum())


@pytest.mark.parametrize('name', sorted(ALL))
def test_held_out_rows_are_decided_and_fits_have_a_stated_tolerance(name):
    """No held-out row has the oracle's p within 1e-4 of 0.5 (the cap on such rows is zero): with weights that agree to the stated
    tolerances the device counts the same rows.  Every job's length has a tolerance in tests/test_gpu_train.py."""
    c = ALL[name]
    for f, (tr, va) in zip(MC.oracle(c), MC.job_rows(c)):
        assert len(f['p_val']) == len(va) > 0
        assert np.abs(f['p_val'] - 0.5).min() >= 1e-4
        assert 0 <= f['val_correct'] <= len(va)
        assert f['n_iter'] == len(f['loss_curve']) <= c['max_iter'] and (f['n_iter'] > 0) == (len(tr) > 0)
        MC.tolerances(f['n_iter'])
        for k in ('W1', 'b1', 'W2', 'loss_curve'):
            assert np.isfinite(f[k]).all()
