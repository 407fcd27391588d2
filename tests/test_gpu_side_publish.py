"""A pipelined pass whose packed block is too small, repeated while the GPU is busy -- against the C oracle, with the side grid
bigger than the chip holds and with passes in flight behind it.

The side stream's one kernel (k2_mlp<.., PACK>, mc_classify.hip) sends the pass's counters to the host from the workgroup that is
through last; k_pack sends them from its workgroup 0.  A pass whose counters never reach the host must be an error
(mc_wait_records_begin), not a copy-out sized by the counters of an earlier pass.  The dense cases force a side grid of 4096
workgroups (MCALLER_SIDE_GRID): most of them start only when others are through, some beside the next pass's fused scan.  Every case
also asks the library how the pass ran (mc_last_pass_info): repeated by the synchronous path, or not."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

FT = 960            # rows per piece of the fused dense pass (mc_fused.hip): the side grid is at most the pieces
GRID = 4096
_tables = {}


@pytest.fixture()
def dev():
    from mcaller_amd.device import Device
    d = Device(0)           # (a context of its own: what an earlier pass made the block grow to decides whether a pass fits)
    yield d
    d.close()


def nn_model():
    from mcaller_amd.extract_contexts import submodel_setup
    from mcaller_amd.model_io import load_model_file, shipped_model
    _, weights, _, soc = submodel_setup(load_model_file(shipped_model('r95_twobase_model_NN_6_m6A')), 'A')
    return weights, soc


def case_table(motif, n_rows, stalls=False):
    """-> table, qual, reference arrays, oracle records (unscored).  Cached: the oracle's prob is set by every user."""
    key = (motif, n_rows, stalls)
    if key not in _tables:
        from mcaller_amd import synth
        codes = synth.genome(length=400000, seed=8)
        ref = synth.SynthRef(codes, motif=motif)
        table, qual = synth.make_table(n_rows, seed=81, codes=codes, read_len=(1000, 4000))
        if stalls:            # (slots of more than 128 events: the pass is marked irregular as well)
            from tests.test_gpu_parity import with_stalls
            table = with_stalls(table, 400, (129, 160, 200, 300), seed=5)
        arrays = ref.device_arrays()
        _tables[key] = (table, qual, arrays, H.oracle_records(table, arrays, qual, 6, 0, 0.0))
    return _tables[key]


def dense_table(stalls=False):
    table, qual, arrays, orc = case_table('A', 5000000, stalls)
    assert -(-table.n_rows // FT) >= GRID          # (pieces: the forced side grid really is GRID workgroups)
    assert orc.n > 400000
    return table, qual, arrays, orc


def handed_out(d, orc, rerun, score=True, tol=1e-6, fused=True):
    rec = d.wait()
    room, was = d.last_pass_info()
    assert was == rerun, (room, was)
    if fused and not rerun:
        assert room > 0, room                      # (the fused dense pass: its side kernel is the one under test)
    if score:
        H.assert_records_equal(rec, orc, 6, prob_tol=tol)
    else:
        rec.prob[:rec.n] = np.nan
        orc.prob[:orc.n] = np.nan
        H.assert_records_equal(rec, orc, 6)


def small_block_then_four(d, orc, score=True, tol=1e-6):
    """The first pass finds its packed block too small and is repeated; four in flight behind it have the grown block."""
    d.run_async(6, 0, 0.0, score=score)
    handed_out(d, orc, True, score, tol)
    for _ in range(4):
        d.run_async(6, 0, 0.0, score=score)
    for _ in range(4):
        handed_out(d, orc, False, score, tol)


def set_side_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv('MCALLER_SIDE_GRID', raising=False)
    else:
        monkeypatch.setenv('MCALLER_SIDE_GRID', str(grid))


@pytest.mark.parametrize('grid', [None, GRID])
def test_dense_pass_with_a_small_block_and_an_oversubscribed_side_grid(dev, grid, monkeypatch):
    """-m A, 5 x 10^6 rows, the shipped NN (the 7-input fast instance of the side kernel)."""
    table, qual, arrays, orc = dense_table()
    weights, soc = nn_model()
    H.oracle_score(orc, table, qual, weights, soc, 6)
    monkeypatch.setenv('MCALLER_PACK_RECORDS', '100')
    set_side_grid(monkeypatch, grid)
    dev.set_reference(arrays)
    dev.set_mlp(weights, soc)
    dev.upload_table_async(table, qual)
    small_block_then_four(dev, orc)


@pytest.mark.parametrize('score', [True, False])
def test_dense_pass_with_a_small_block_fp64_and_features_only(dev, score, monkeypatch):
    """The other instances of the side kernel: fp64 throughout (MCALLER_MLP_FP64, read when the model is set) and no classifier."""
    table, qual, arrays, orc = dense_table()
    weights, soc = nn_model()
    H.oracle_score(orc, table, qual, weights, soc, 6)
    monkeypatch.setenv('MCALLER_MLP_FP64', '1')
    monkeypatch.setenv('MCALLER_PACK_RECORDS', '100')
    set_side_grid(monkeypatch, GRID)
    dev.set_reference(arrays)
    dev.set_mlp(weights, soc)
    dev.upload_table_async(table, qual)
    small_block_then_four(dev, orc, score=score, tol=1e-9)


def test_sparse_pass_with_a_small_block_and_five_passes_behind_it(dev, monkeypatch):
    """GATC, 10^7 rows: the sparse side grid stays within the chip, so the pressure comes from six passes in flight -- the first
    one's side kernel runs beside the later passes' scans.  Only the first pass has a small block."""
    table, qual, arrays, orc = case_table('GATC', 10000000)
    weights, soc = nn_model()
    H.oracle_score(orc, table, qual, weights, soc, 6)
    assert orc.n > 10000
    dev.set_reference(arrays)
    dev.set_mlp(weights, soc)
    dev.upload_table_async(table, qual)
    monkeypatch.setenv('MCALLER_PACK_RECORDS', '100')
    dev.run_async(6, 0, 0.0, score=True)
    monkeypatch.delenv('MCALLER_PACK_RECORDS')     # (read per pass: the next five get a block for all their records)
    for _ in range(5):
        dev.run_async(6, 0, 0.0, score=True)
    handed_out(dev, orc, True, fused=False)
    for _ in range(5):
        handed_out(dev, orc, False, fused=False)


def test_a_pass_too_big_for_its_block_and_irregular(dev, monkeypatch):
    """A pass whose block is too small AND that holds slots of more than 128 events (irregular: the walk is the synchronous
    path's): repeated once, equal."""
    table, qual, arrays, orc = dense_table(stalls=True)
    weights, soc = nn_model()
    H.oracle_score(orc, table, qual, weights, soc, 6)
    monkeypatch.setenv('MCALLER_PACK_RECORDS', '100')
    set_side_grid(monkeypatch, GRID)
    dev.set_reference(arrays)
    dev.set_mlp(weights, soc)
    dev.upload_table_async(table, qual)
    dev.run_async(6, 0, 0.0, score=True)
    handed_out(dev, orc, True)


def test_record_overflow_with_an_oversubscribed_side_grid(dev, monkeypatch):
    """A piece's room forced too small (MCALLER_FUSED_ROOM): the fused pass overflows its records before the side kernel starts,
    every one of its 4096 workgroups returns at entry and workgroup 0 sends the counters.  Repeated, equal; the next pass, with
    the room the library picks, is not."""
    table, qual, arrays, orc = dense_table()
    weights, soc = nn_model()
    H.oracle_score(orc, table, qual, weights, soc, 6)
    set_side_grid(monkeypatch, GRID)
    monkeypatch.setenv('MCALLER_FUSED_ROOM', '16')
    dev.set_reference(arrays)
    dev.set_mlp(weights, soc)
    dev.upload_table_async(table, qual)
    dev.run_async(6, 0, 0.0, score=True)
    handed_out(dev, orc, True)
    assert dev.last_pass_info() == (16, True)
    monkeypatch.delenv('MCALLER_FUSED_ROOM')
    dev.run_async(6, 0, 0.0, score=True)
    dev.run_async(6, 0, 0.0, score=True)
    handed_out(dev, orc, False)
    handed_out(dev, orc, False)


@pytest.mark.parametrize('motif,n_rows,fused', [('A', 1000000, True), ('GATC', 4000000, False)])
def test_k_pack_with_a_small_block(dev, motif, n_rows, fused, monkeypatch):
    """A forest (k3_forest, then k_pack_count / k_pack: workgroup 0 sends the counters): the first pass with a small block is
    repeated, three in flight behind it are not -- dense (holes) and sparse."""
    from tests import clf_cases as CC
    rng = np.random.default_rng(77)
    thr, _ = CC.threshold_pool(rng, 7, scale=6.0)
    forests = CC.forests(rng, 7, (20, 65, 1), depth=(0, 14), thr=thr)
    soc = np.full(256, 255, dtype=np.uint8)
    for i, c in enumerate('ACGT'):
        soc[ord(c)] = i % 3
    monkeypatch.setenv('MCALLER_PACK_RECORDS', '100')
    table, qual, arrays, orc = case_table(motif, n_rows)
    H.oracle_score(orc, table, qual, forests, soc, 6)
    assert np.isfinite(orc.prob[:orc.n]).sum() > 1000
    dev.set_reference(arrays)
    dev.set_classifier(forests, soc)
    dev.upload_table_async(table, qual)
    dev.run_async(6, 0, 0.0, score=True)
    handed_out(dev, orc, True, tol=0.0, fused=fused)
    for _ in range(3):
        dev.run_async(6, 0, 0.0, score=True)
    for _ in range(3):
        handed_out(dev, orc, False, tol=0.0, fused=fused)


def test_streamed_rows_when_a_shard_is_repeated(tmp_path):
    """-m A streamed in six shards with a small packed block: the first shard's pass is repeated (its rows come from the host
    formatter), later shards' rows are written on the device -- the file is the unstreamed run's byte for byte."""
    from tests.test_gpu_rowtext import MODEL, run_cli, write_case
    d = str(tmp_path)
    paths, rows = write_case(d, 31, n_reads=48, edge_reads=False, decimals=(2,))
    want, _, _ = run_cli(paths, 'A', {'MCALLER_NO_STREAM': '1'})
    assert want.count(b'\n') > 1000
    out = paths['tsv'][:-4] + '.diffs.6'
    os.remove(out)
    env = dict(os.environ, MCALLER_STREAM_SHARDS='6', MCALLER_PACK_RECORDS='20', MCALLER_VERBOSE='1')
    for k in ('MCALLER_NO_STREAM', 'MCALLER_DEVICE_ROWS', 'MCALLER_ROW_TEXT_BLOCKS'):
        env.pop(k, None)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'mcaller_amd.mCaller', '-m', 'A', '-r', paths['fasta'], '-e', paths['tsv'], '-f', paths['fastq'], '-d', MODEL],
                       cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, 'rb').read() == want
    assert 'pass re-run synchronously (overflow 1' in r.stderr, r.stderr[-2000:]
    said = [l for l in r.stderr.splitlines() if 'rows written on the device for' in l]
    assert said, r.stderr[-2000:]
    assert int(said[-1].split(' for ')[1].split()[0]) >= 1
