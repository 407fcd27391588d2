"""RF / LR / NBC / SVM on the GPU (k3_forest, k3_simple, k3_svm) at the shapes and on the passes the MLP is tested on: synthetic
models of 2 .. 9 inputs (tests/clf_cases.py) through the estimator protocol with edge probes, flush records at k = 2, 4, 6, 8 on a
sparse and a dense reference and every pass type, and the command line at -n 4 with five-input model files
(tests/golden/shapes/).  References: the C oracle's forest walk bit for bit, the numpy restatements of LR / NBC to 1e-12 and of
the SVM to 1e-11 (tests/test_clf_shapes.py pins them against scikit-learn)."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest

from oracle import clf_oracle
from tests import clf_cases as CC
from tests import helpers as H
from tests import svm_oracle

pytestmark = pytest.mark.gpu

SHAPES = os.path.join(H.GOLDEN, 'shapes')


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def n_cu():
    """Compute units of device 0 (hipDeviceGetAttribute, hipDeviceAttributeMultiprocessorCount = 63): the library sizes
    k3_forest's grid by them."""
    hip = ctypes.CDLL('libamdhip64.so')
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0 and v.value > 0
    return v.value


def forest_switch():
    """The record count up to which k3_forest walks a record with a wave (mc_launch_classifier's grid: min((n + 3) / 4, 8 CUs);
    four waves per workgroup, 16 records per wave): 131 072 on a 256-CU MI355X."""
    return 8 * n_cu() * 4 * 16


# ---- the estimator protocol ----

FOREST_SETS = {2: (1, 63, 65), 5: (64, 130, 1), 7: (65, 63, 64), 9: (130, 1, 65)}


@pytest.mark.parametrize('n_in', [2, 5, 7, 9])
def test_forest_edges_and_both_shapes(dev, n_in):
    """Ragged sub-models of 1, 63, 64, 65 and 130 trees of depth 0 .. 20, zero-sum leaves, probes on the thresholds, the index past
    the sub-models among them -- a wave per record (few rows and exactly at the switch) and a lane per record (one past it)."""
    forests, X, sub = CC.forest_case(200 + n_in, n_in, FOREST_SETS[n_in], depth=(0, 20))
    dev.set_classifier(forests, np.full(256, 255, dtype=np.uint8))
    edge = forest_switch()
    for n in (64, len(X), edge, edge + 1):
        reps = -(-n // len(X))
        Xn, sn = np.tile(X, (reps, 1))[:n], np.tile(sub, reps)[:n]
        got = dev.classifier_forward(Xn, sn)
        want = H.oracle_forest_forward(forests, Xn, sn)
        assert np.array_equal(np.isnan(got), np.isnan(want)), n
        ok = ~np.isnan(want)
        assert ok.any() and np.array_equal(got[ok], want[ok]), (n, np.abs(got[ok] - want[ok]).max())
    print('n_in %d: trees %s, rows 64 .. %d (switch at %d)' % (n_in, FOREST_SETS[n_in], edge + 1, edge))


def test_forest_a_million_rows(dev):
    rng = np.random.default_rng(9)
    thr, vals = CC.threshold_pool(rng, 5)
    forests = CC.forests(rng, 5, (1, 63, 65), depth=(0, 10), thr=thr)
    X = CC.forest_probes(rng, vals, 1000000)
    sub = rng.integers(0, 4, size=len(X)).astype(np.uint8)
    dev.set_classifier(forests, np.full(256, 255, dtype=np.uint8))
    got = dev.classifier_forward(X, sub)
    want = H.oracle_forest_forward(forests, X, sub)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])


SVM_SV = (1, 255, 256, 257, 512, 3, 64, 100)        # K3S_TILE = 256; eight sub-models (K3S_MAXM), the sixth with gamma = 0


@pytest.mark.parametrize('n_in', [2, 5, 7, 9])
def test_svm_tiles_eight_submodels_and_the_band(dev, n_in):
    """Eight sub-models interleaved record by record (and the index 8: NaN), support-vector counts around the LDS tile, gamma = 0,
    100 003 rows; probes in the band (p = 1/2 exactly), at its edges and past the 1e-7 clamp.  n_in != 7: k3_svm<0>."""
    rng = np.random.default_rng(300 + n_in)
    models = [CC.svm_model(rng, n_in, n, gamma=0.0) if i == 5 else CC.svm_scaled(rng, n_in, n) for i, n in enumerate(SVM_SV)]
    n = 100003
    X = rng.normal(0, 2.0, size=(n, n_in))
    share = np.array([1.0 if m.n_sv < 255 else 0.05 for m in models] + [1.0])      # (the numpy reference's time: the large sets
    sub = rng.choice(9, size=n, p=share / share.sum()).astype(np.uint8)             # get fewer rows, a few in every workgroup)
    at = 0
    for i, w in enumerate(models):
        P = CC.svm_band_probes(rng, w)
        X[at:at + len(P)] = P
        sub[at:at + len(P)] = i
        at += len(P)
    order = rng.permutation(n)
    X, sub = X[order], sub[order]
    dev.set_classifier(models, np.full(256, 255, dtype=np.uint8))
    got = dev.classifier_forward(X, sub)
    want = svm_oracle.forward(models, X, sub)
    err = CC.assert_matches(got, want, 1e-11)
    assert np.isnan(got).sum() == (sub == 8).sum() > 0
    assert (want == 0.5).sum() >= 8 * 3 and (want > 0.9).any() and (want < 0.1).any()
    print('n_in %d: k3_svm<%d>, %d rows, largest |dp| %.3g' % (n_in, 7 if n_in == 7 else 0, n, err))


@pytest.mark.parametrize('n_in', [2, 5, 7, 9])
def test_logistic_saturation_and_exact_half(dev, n_in):
    rng = np.random.default_rng(400 + n_in)
    models = CC.logistic_models(rng, n_in, 3)
    half, x_half = CC.logistic_exact_half(n_in)
    models.append(half)
    X = [CC.logistic_probes(rng, w) for w in models[:3]] + [x_half]
    sub = np.concatenate([np.full(len(x), i) for i, x in enumerate(X)] + [np.full(5, 4)]).astype(np.uint8)
    X = np.concatenate(X + [np.zeros((5, n_in))])
    dev.set_classifier(models, np.full(256, 255, dtype=np.uint8))
    got = dev.classifier_forward(X, sub)
    want = clf_oracle.forward(models, X, sub)
    CC.assert_matches(got, want, 1e-12)
    assert (want == 0.0).any() and (want == 1.0).any() and (want == 0.5).any() and np.isnan(want).sum() == 5


@pytest.mark.parametrize('n_in', [2, 5, 7, 9])
def test_gnb_saturation_and_ties(dev, n_in):
    rng = np.random.default_rng(500 + n_in)
    models = CC.gnb_models(rng, n_in, 2) + [CC.gnb_tiny_var(rng, n_in)]
    tie, x_tie = CC.gnb_tie(rng, n_in)
    far, x_far = CC.gnb_tie(rng, n_in, var=1e-6)          # (|jll| ~ 1e6 with p in the middle: numpy's order of the sums shows)
    models += [tie, far]
    X = [CC.gnb_probes(rng, w) for w in models[:3]] + [np.concatenate([x_tie, CC.gnb_probes(rng, tie, 20)]),
                                                       np.concatenate([x_far, CC.gnb_near_tie_probes(rng, far, x_far, 200)])]
    sub = np.concatenate([np.full(len(x), i) for i, x in enumerate(X)]).astype(np.uint8)
    X = np.concatenate(X)
    dev.set_classifier(models, np.full(256, 255, dtype=np.uint8))
    got = dev.classifier_forward(X, sub)
    want = clf_oracle.forward(models, X, sub)
    err = CC.assert_matches(got, want, 1e-12)
    assert (want == 0.0).any() and (want == 1.0).any()
    t = int(np.nonzero(sub == 3)[0][0])
    assert abs(want[t] - 0.5) <= 1e-15 and got[t] == want[t]       # the tie: the label is p >= 0.5 of the same rounding
    print('n_in %d: largest |dp| %.3g' % (n_in, err))


# ---- flush records: k = 2, 4, 6, 8, sparse and dense, every pass type ----

def hot_models(kind, k, seed):
    rng = np.random.default_rng(seed)
    n_in = k + 1
    if kind == 'forest':
        thr, _ = CC.threshold_pool(rng, n_in, scale=6.0)
        return CC.forests(rng, n_in, (20, 65, 1), depth=(0, 14), thr=thr)
    if kind == 'logistic':
        return CC.logistic_models(rng, n_in, 3)
    if kind == 'gnb':
        return CC.gnb_models(rng, n_in, 3)
    return [CC.svm_model(rng, n_in, n, gamma=0.08) for n in (300, 1, 257)]


def scored(rec):
    r = rec.by_record() if getattr(rec, 'call_row', None) is not None else rec
    return int(np.isfinite(r.prob[:r.n]).sum())


TOL = {'forest': 0.0, 'logistic': 1e-12, 'gnb': 1e-12, 'svm': 1e-11}
_tables = {}


def hot_table(motif, k):
    from mcaller_amd import synth
    key = (motif, k)
    if key not in _tables:
        codes = synth.genome(length=120000, seed=40)
        ref = synth.SynthRef(codes, motif=motif)
        table, qual = synth.make_table(160000 if motif == 'GATC' else 60000, seed=41, codes=codes, read_len=(1500, 6000))
        arrays = ref.device_arrays()
        _tables[key] = (table, qual, arrays, H.oracle_records(table, arrays, qual, k, 0, 0.0))
    return _tables[key]


@pytest.mark.parametrize('kind', ['forest', 'logistic', 'gnb', 'svm'])
@pytest.mark.parametrize('k', [2, 4, 6, 8])
def test_flush_records_every_pass(dev, kind, k, monkeypatch):
    """The synchronous pass (scan + emit), one pipelined pass, four in flight; on the dense reference the pipelined passes are
    the fused kernel (holes in the record slots, the count on the device) and, behind MCALLER_DENSE_FUSED=0, the pair."""
    weights = hot_models(kind, k, 600 + 10 * k)
    soc = np.full(256, 255, dtype=np.uint8)
    for i, c in enumerate('ACGT'):                # ('M': no sub-model -- NaN on the device, as in the oracle)
        soc[ord(c)] = i % 3
    for motif in ('GATC', 'A'):
        table, qual, arrays, orc = hot_table(motif, k)
        H.oracle_score(orc, table, qual, weights, soc, k)
        n_scored = int(np.isfinite(orc.prob[:orc.n]).sum())
        assert n_scored > (20 if motif == 'GATC' else 2000), (motif, n_scored)
        dev.set_reference(arrays)
        dev.set_classifier(weights, soc)
        dev.upload_table_async(table, qual)
        rec = dev.extract(k, 0, 0.0)
        H.assert_records_equal(rec, orc, k, prob_tol=TOL[kind])
        assert scored(rec) == n_scored
        dev.run_async(k, 0, 0.0)
        rec = dev.wait()
        H.assert_records_equal(rec, orc, k, prob_tol=TOL[kind])
        assert scored(rec) == n_scored
        if motif == 'A':
            assert dev.last_pass_info()[0] > 0                        # (the fused dense pass)
        for _ in range(4):
            dev.run_async(k, 0, 0.0)
        for _ in range(4):
            rec = dev.wait()
            H.assert_records_equal(rec, orc, k, prob_tol=TOL[kind])
            assert scored(rec) == n_scored
        if motif == 'A':
            monkeypatch.setenv('MCALLER_DENSE_FUSED', '0')
            dev.run_async(k, 0, 0.0)
            rec = dev.wait()
            assert dev.last_pass_info() == (0, False)
            H.assert_records_equal(rec, orc, k, prob_tol=TOL[kind])
            assert scored(rec) == n_scored
            monkeypatch.delenv('MCALLER_DENSE_FUSED')
    if kind == 'svm' and k + 1 != 7:
        print('k3_svm<0>: %d inputs, records scored' % (k + 1))


def test_forest_lane_per_record_inside_a_dense_pass(dev):
    """One dense pass with more forest records than k3_forest walks a wave at a time: the lane-per-record shape on the hot path,
    synchronous and pipelined (there the count is on the device, the grid sized by the capacity)."""
    from mcaller_amd import synth
    k = 6
    codes = synth.genome(length=300000, seed=42)
    ref = synth.SynthRef(codes, motif='A')
    table, qual = synth.make_table(2000000, seed=43, codes=codes)
    arrays = ref.device_arrays()
    weights = hot_models('forest', k, 700)
    soc = np.full(256, 255, dtype=np.uint8)
    for i, c in enumerate('ACGTM'):
        soc[ord(c)] = i % 3
    orc = H.oracle_records(table, arrays, qual, k, 0, 0.0)
    H.oracle_score(orc, table, qual, weights, soc, k)
    n_scored = int(np.isfinite(orc.prob[:orc.n]).sum())
    assert n_scored > forest_switch(), (n_scored, forest_switch())
    dev.set_reference(arrays)
    dev.set_classifier(weights, soc)
    dev.upload_table_async(table, qual)
    rec = dev.extract(k, 0, 0.0)
    H.assert_records_equal(rec, orc, k, prob_tol=0.0)
    assert scored(rec) == n_scored
    dev.run_async(k, 0, 0.0)
    rec = dev.wait()
    H.assert_records_equal(rec, orc, k, prob_tol=0.0)
    assert scored(rec) == n_scored
    print('%d forest records in one pass (switch at %d)' % (n_scored, forest_switch()))


# ---- the command line at -n 4 ----

_inputs = {}


def cli_inputs(tmp_path_factory):
    from mcaller_amd import synth
    if 'paths' not in _inputs:
        codes = synth.genome(length=150000, seed=44)
        table, qual = synth.make_table(150000, seed=45, codes=codes, read_len=(1500, 6000))
        _inputs['paths'] = synth.write_inputs(table, qual, codes, str(tmp_path_factory.mktemp('shapes_cli')))
    return _inputs['paths']


def run_cli(paths, model, tag, motif, env):
    from mcaller_amd import mCaller
    keys = ('MCALLER_NO_STREAM', 'MCALLER_STREAM_SHARDS', 'MCALLER_DEVICE_ROWS')
    saved = {key: os.environ.pop(key, None) for key in keys}
    os.environ.update(env)
    out = paths['tsv'][:-4] + '.diffs.4'
    if os.path.exists(out):
        os.remove(out)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mCaller.main(['-m', motif, '-n', '4', '-r', paths['fasta'], '-e', paths['tsv'], '-f', paths['fastq'], '-d', model,
                          '-c', 'RF' if tag.startswith('RF') else tag])
    finally:
        for key in keys:
            os.environ.pop(key, None)
            if saved[key] is not None:
                os.environ[key] = saved[key]
    return open(out, 'rb').read()


def reference_p(ms, keys, feats):
    p = np.empty(len(feats))
    for key in set(keys):
        sel = np.array([x == key for x in keys])
        w = ms.models[key]
        if w.kind == 'forest':
            p[sel] = H.oracle_forest_forward([w], feats[sel], np.zeros(int(sel.sum()), dtype=np.uint8))
        elif w.kind == 'svm':
            p[sel] = svm_oracle.proba(w, feats[sel])
        else:
            p[sel] = clf_oracle.forward([w], feats[sel], np.zeros(int(sel.sum()), dtype=np.uint8))
    return p


@pytest.mark.parametrize('tag', ['RF', 'RF4', 'LR', 'NBC', 'SVM'])
def test_cli_five_input_models(tag, tmp_path_factory):
    """-n 4 -m GATC and -m A with a five-input model file: every row's label and printed probability are the reference's on the
    features the row prints; the bytes the same with one pass, three streamed shards and the host's row formatter."""
    from mcaller_amd.model_io import load_model_file
    paths = cli_inputs(tmp_path_factory)
    model = os.path.join(SHAPES, 'shapes_twobase_model_%s_4_m6A.pkl' % tag)
    ms = load_model_file(model)
    ties = {'half_cent': 0, 'half': 0, 'one': 0}
    for motif in ('GATC', 'A'):
        one = run_cli(paths, model, tag, motif, {'MCALLER_NO_STREAM': '1'})
        rows = [line.split('\t') for line in one.decode().splitlines()]
        assert len(rows) > (100 if motif == 'GATC' else 5000), (motif, len(rows))
        feats = np.array([[float(v) for v in r[4].split(',')] for r in rows])
        assert feats.shape[1] == 5
        keys = ['MG' if r[3][3:5] == 'MG' else 'MH' for r in rows]
        p = reference_p(ms, keys, feats)
        for r, pi in zip(rows, p):
            assert r[7] == str(np.round(pi, 2)) and r[6] == ('m6A' if pi >= 0.5 else 'A'), (r, pi)
        ties['half_cent'] += int(((p * 100.0) % 1.0 == 0.5).sum())
        ties['half'] += int((p == 0.5).sum())
        ties['one'] += int((p == 1.0).sum())
        assert run_cli(paths, model, tag, motif, {'MCALLER_STREAM_SHARDS': '3'}) == one, motif
        assert run_cli(paths, model, tag, motif, {'MCALLER_DEVICE_ROWS': '0'}) == one, motif
    if tag == 'RF4':                               # four trees: the printed ties happen
        assert all(v > 0 for v in ties.values()), ties
    print('%s: ties %s' % (tag, ties))
