"""`-c SVM` on the GPU (k3_svm): the estimator protocol against scikit-learn's captured predict_proba, a ragged synthetic model
against the numpy restatement, flush records of one, pipelined and overlapping passes, and the command line."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import svm_oracle

pytestmark = pytest.mark.gpu

SVM = os.path.join(H.GOLDEN, 'svm')
TWOBASE = os.path.join(SVM, 'svm_twobase_model_SVM_6_m6A.pkl')
GENERAL = os.path.join(SVM, 'svm_model_SVM_6_m6A.pkl')


def meta():
    return json.load(open(os.path.join(SVM, 'svm_meta.json')))


def setup(path):
    from mcaller_amd.extract_contexts import submodel_setup
    from mcaller_amd.model_io import load_model_file
    ms = load_model_file(path)
    _, models, _, soc = submodel_setup(ms, 'A')
    return ms, models, soc


def score_records(rec, table, qual, models, soc, k):
    """Probabilities of the records the device scores (no MC_I_TOO_MANY / MC_I_EDGE, a known sub-model), by the numpy
    restatement; NaN elsewhere, as on the device."""
    from mcaller_amd import _lib
    n = rec.n
    info = rec.info[:n]
    sub = soc[(info >> _lib.I_NEXT_SHIFT) & 0xFF].astype(np.int64)
    sub[(info & (_lib.I_TOO_MANY | _lib.I_EDGE)) != 0] = 255
    X = np.zeros((n, k + 1))
    X[:, :k] = rec.feats[:n * k].reshape(n, k)
    X[:, k] = np.asarray(qual, dtype=np.float64)[table.seg_read[rec.site_seg[:n]]]
    rec.prob[:n] = svm_oracle.forward(models, X, sub)


@pytest.mark.parametrize('path', [TWOBASE, GENERAL])
def test_forward_matches_known_answers(path):
    from mcaller_amd.device import Device
    ms, models, soc = setup(path)
    m = meta()
    dev = Device(0)
    dev.set_classifier(models, soc)
    for i, key in enumerate(ms.keys()):
        X = np.array(m['probes'][key])
        p = dev.classifier_forward(X, np.full(len(X), i, dtype=np.uint8))
        want = np.array(m['known_answers'][key])
        assert np.abs(p - want).max() <= 1e-12, (key, np.abs(p - want).max())
        assert all(p[j] == 0.5 for j in m['in_band'][key])
        assert all(p[j] != 0.5 for j in m['near_band'][key])
    dev.close()


def test_ragged_model_on_mixed_rows():
    """3000 and 7001 support vectors (several LDS tiles, the last one partial), 10^5 rows of interleaved sub-models, the KeyError
    index among them: the numpy restatement to 1e-11, NaN in the same places."""
    from mcaller_amd.device import Device
    from mcaller_amd.model_io import SVMWeights
    rng = np.random.default_rng(5)

    def rows(n):
        return np.concatenate([rng.normal(0, 2.5, size=(n, 6)), rng.uniform(6, 12, size=(n, 1))], axis=1)
    models = [SVMWeights(rows(n_sv), rng.uniform(-1, 1, size=n_sv), g, b, a, bb, ['A', 'm6A'])
              for n_sv, g, b, a, bb in ((3000, 0.021, 0.3, -0.35, 0.05), (7001, 0.017, -0.2, -0.25, -0.1))]
    X = rows(100000)
    sub = rng.choice([0, 1, 1, 2], size=len(X)).astype(np.uint8)        # 2: no such sub-model (the reference's KeyError path)
    soc = np.full(256, 255, dtype=np.uint8)
    dev = Device(0)
    dev.set_classifier(models, soc)
    p = dev.classifier_forward(X, sub)
    dev.close()
    want = svm_oracle.forward(models, X, sub)
    assert np.array_equal(np.isnan(p), np.isnan(want)) and np.isnan(p).sum() == (sub == 2).sum()
    ok = ~np.isnan(want)
    assert np.abs(p[ok] - want[ok]).max() <= 1e-11, np.abs(p[ok] - want[ok]).max()
    assert (want[ok] > 0.9).any() and (want[ok] < 0.1).any()


def test_flush_records_one_pass_pipelined_and_four_in_flight():
    from mcaller_amd import synth
    from mcaller_amd.device import Device
    _, models, soc = setup(TWOBASE)
    codes = synth.genome(length=300000, seed=4)
    ref = synth.SynthRef(codes)
    table, qual = synth.make_table(300000, seed=8, codes=codes)
    dev = Device(0)
    dev.set_classifier(models, soc)
    dev.set_reference(ref.device_arrays()); dev.upload_table(table); dev.set_read_quality(qual)
    orc = H.oracle_records(table, ref.device_arrays(), qual, 6, 0, 0.0)
    score_records(orc, table, qual, models, soc, 6)
    rec = dev.extract(6, 0, 0.0)
    H.assert_records_equal(rec, orc, 6, prob_tol=1e-12)
    assert np.isfinite(rec.prob[:rec.n]).sum() > 100
    dev.run_async(6, 0, 0.0)
    H.assert_records_equal(dev.wait(), orc, 6, prob_tol=1e-12)
    for _ in range(4):
        dev.run_async(6, 0, 0.0)
    for _ in range(4):
        H.assert_records_equal(dev.wait(), orc, 6, prob_tol=1e-12)
    dev.close()


def run_cli(paths, model, env):
    from mcaller_amd import mCaller
    keys = ('MCALLER_NO_STREAM', 'MCALLER_STREAM_SHARDS')
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    out = paths['tsv'][:-4] + '.diffs.6'
    if os.path.exists(out):
        os.remove(out)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mCaller.main(['-m', 'GATC', '-r', paths['fasta'], '-e', paths['tsv'], '-f', paths['fastq'], '-d', model, '-c', 'SVM'])
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return open(out, 'rb').read()


def check_rows(text, ms):
    """Every row's label and printed probability are the numpy restatement's on the features the row prints."""
    rows = [l.split('\t') for l in text.decode().splitlines()]
    assert len(rows) > 100
    feats = np.array([[float(v) for v in r[4].split(',')] for r in rows])
    keys = ['general'] * len(rows) if not ms.twobase else ['MG' if r[3][5:7] == 'MG' else 'MH' for r in rows]
    p = np.empty(len(rows))
    for key in set(keys):
        sel = np.array([k == key for k in keys])
        p[sel] = svm_oracle.proba(ms.models[key], feats[sel])
    for r, pi in zip(rows, p):
        assert abs(float(np.round(pi, 2)) - float(r[7])) < 1e-9 and r[6] == ('m6A' if pi >= 0.5 else 'A'), r


@pytest.mark.parametrize('model', [TWOBASE, GENERAL])
def test_cli_with_an_svm_model_file(tmp_path, model):
    from mcaller_amd import synth
    from mcaller_amd.model_io import load_model_file
    codes = synth.genome(length=200000, seed=27)
    table, qual = synth.make_table(250000, seed=11, codes=codes, read_len=(1500, 6000))
    paths = synth.write_inputs(table, qual, codes, str(tmp_path))
    one = run_cli(paths, model, {'MCALLER_NO_STREAM': '1'})
    check_rows(one, load_model_file(model))
    assert run_cli(paths, model, {'MCALLER_STREAM_SHARDS': '3'}) == one


def test_train_svm_then_score_with_the_written_file(tmp_path):
    """`--train -c SVM` (scikit-learn's fit, train_model.py:51-53) on the committed training rows, then the file it wrote scored on the
    GPU: the numpy restatement's probabilities on the rows it was fitted on.  (A file written by --train is a dict keyed 'general',
    which the two-base sub-model keys of a calling run do not name -- the reference's KeyError exit -- so it is scored here through
    the estimator protocol.)"""
    pytest.importorskip('sklearn')
    import shutil
    from mcaller_amd import mCaller
    from mcaller_amd.device import Device
    from mcaller_amd.load_mCaller_data import tsv2matrix
    from mcaller_amd.model_io import load_model_file
    td = H.testdata_paths(str(tmp_path))
    rows = str(tmp_path / 'training_rows.train')
    shutil.copy(os.path.join(H.GOLDEN, 'train', 'training_rows.train'), rows)
    model = str(tmp_path / 'model_SVM_6_m6A.pkl')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '--train',
                      '--training_tsv', rows, '-c', 'SVM', '-d', model])
    assert 'SVM general model scores: ' in buf.getvalue()
    ms = load_model_file(model)
    assert ms.keys() == ['general'] and ms.models['general'].kind == 'svm'
    sig, _ = tsv2matrix(rows, 'A')
    X = np.array([f for lab in sig['general'].values() for f in lab])
    w = ms.models['general']
    dev = Device(0)
    dev.set_classifier([w], np.zeros(256, dtype=np.uint8))
    p = dev.classifier_forward(X, np.zeros(len(X), dtype=np.uint8))
    dev.close()
    want = svm_oracle.proba(w, X)
    assert len(X) > 20 and np.abs(p - want).max() <= 1e-12
