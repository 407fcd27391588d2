"""The array-aware side of `--train` behind load_mCaller_data.tsv2matrix_device (no GPU): balancing over array leaves picks the rows
balanced_rows picks, train_classifier prints the same three lines for list leaves and array leaves, the folds of cv_jobs do not
depend on whether the contexts are str or an 'S' array; and MCALLER_TRAIN_ROWS_DEVICE=0 is the host function."""
import contextlib
import io
import os

import numpy as np
import pytest

from tests import helpers as H

ROWS = os.path.join(H.GOLDEN, 'train', 'training_rows.train')


def as_arrays(sig, grp):
    width = max([len(r) for rows in sig.values() for r in rows] + [0])
    return ({label: np.asarray(rows, dtype=np.float64).reshape(len(rows), width) for label, rows in sig.items()},
            {label: np.asarray([c.encode('ascii') for c in rows], dtype='S') if rows else np.zeros(0, dtype='S1') for label, rows in grp.items()})


def made(sizes, seed):
    rng = np.random.RandomState(seed)
    sig = {label: [[float(v) for v in np.round(rng.randn(6), 4)] for _ in range(n)] for label, n in sizes}
    grp = {label: [''.join(rng.choice(list('ACGTM'), size=rng.choice((5, 11)))) for _ in range(n)] for label, n in sizes}
    return sig, grp


@pytest.mark.parametrize('sizes', [(('m6A', 9), ('A', 14)), (('A', 14), ('m6A', 9)), (('A', 7), ('m6A', 7)), (('m6A', 12), ('A', 5), ('unsure', 8)),
                                   (('m6A', 4), ('A', 0)), (('only', 3),)])
def test_balanced_arrays_equals_balanced_rows(sizes):
    from mcaller_amd.train_model import balanced_arrays, balanced_rows
    sig, grp = made(sizes, len(sizes) + sizes[0][1])
    labs, sigs, grps = balanced_rows(sig, grp)
    a_sig, a_grp = as_arrays(sig, grp)
    a_labs, a_sigs, a_grps = balanced_arrays(a_sig, a_grp)
    assert list(a_labs) == labs
    assert isinstance(a_sigs, np.ndarray) and a_sigs.dtype == np.float64 and a_sigs.tolist() == sigs
    assert [c.decode('ascii') for c in a_grps.tolist()] == grps


def test_train_classifier_prints_the_same_lines_for_arrays(tmp_path, monkeypatch):
    from mcaller_amd import train_model
    from mcaller_amd.load_mCaller_data import tsv2matrix
    from tests.test_simple_fit import OracleDevice
    monkeypatch.setenv('MCALLER_SEED', '5')
    real = train_model.fit_nb_on_gpu
    seen = []

    def fit(labs, sigs, grps, use_groups, device=None):
        seen.append(type(sigs))
        return real(labs, sigs, grps, use_groups, device=OracleDevice())

    monkeypatch.setattr(train_model, 'fit_nb_on_gpu', fit)
    sig, grp = tsv2matrix(ROWS, 'A')
    a_sig, a_grp = as_arrays(sig['general'], grp['general'])
    said = []
    for s, g, name in ((sig, grp, 'lists'), ({'general': a_sig}, {'general': a_grp}, 'arrays')):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            train_model.train_classifier(s, g, str(tmp_path / (name + '.npz')), 'NBC')
        said.append(buf.getvalue())
    assert said[0] == said[1]
    labs, sigs, grps = train_model.balanced_rows(sig['general'], grp['general'])
    assert said[1].split('\n')[:3] == [str(labs[:10]), str(sigs[:10]), str(grps[:10])]
    assert seen == [list, np.ndarray]                         # the matrix of the array path never was a list


def test_cv_jobs_folds_do_not_depend_on_the_group_type(monkeypatch):
    from mcaller_amd import train_model
    from mcaller_amd.load_mCaller_data import tsv2matrix
    monkeypatch.setenv('MCALLER_SEED', '9')
    sig, grp = tsv2matrix(ROWS, 'A')
    labs, sigs, grps = train_model.balanced_rows(sig['general'], grp['general'])
    rng = np.random.RandomState(3)
    cases = [(labs, grps)]
    made_grps = [''.join(rng.choice(list('ACGTM'), size=rng.choice((3, 5, 11)))) for _ in range(400)]      # (prefixes of one another among them)
    made_grps += [g[:3] for g in made_grps[:40]]
    cases.append((['A', 'm6A'] * (len(made_grps) // 2), made_grps))
    for labels, groups in cases:
        as_s = np.asarray([g.encode('ascii') for g in groups], dtype='S')
        c1, y1, jobs1, seeds1 = train_model.cv_jobs(labels, groups, True)
        c2, y2, jobs2, seeds2 = train_model.cv_jobs(labels, as_s, True)
        assert c1 == c2 and (y1 == y2).all() and seeds1 == seeds2
        assert all((a[0] == b[0]).all() and (a[1] == b[1]).all() for a, b in zip(jobs1, jobs2))
        assert (train_model.group_kfold(groups, 5) == train_model.group_kfold(as_s, 5)).all()


def test_the_knob_forces_the_host_function(monkeypatch):
    from mcaller_amd import load_mCaller_data as L
    monkeypatch.setenv('MCALLER_TRAIN_ROWS_DEVICE', '0')
    L.last_load = None
    assert L.tsv2matrix_device(ROWS, 'A') == L.tsv2matrix(ROWS, 'A')
    assert L.last_load == dict(by='host', reason='MCALLER_TRAIN_ROWS_DEVICE=0', n_rows=sum(len(v) for v in L.tsv2matrix(ROWS, 'A')[0]['general'].values()))
