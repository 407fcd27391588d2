"""Narrow records on the device: the sparse MLP passes send their four record columns as 16-bit halves plus a run list
(k1_emit counts the run starts, k2_mlp<.., PACK> packs: csrc/mc_emit.hip, mc_classify.hip; narrow_layout, csrc/mc_dev.h).  The tables of tests/narrow_records.py --
records on both sides of row 65 536; '+' and '-' reads across a reference position that is a multiple of 65 536 with a read under
the quality threshold between them; reads of one record each; between 512 and 1024 records, so that runs start on the first and
the last record of a packing chunk and of a workgroup's range -- on the synchronous pass and on pipelined passes: every pipelined
pass equals the synchronous one and the C oracle, its run list is the numpy encoder's, and what it sent is the layout's size to the
byte.  A pass without a record, a packed block that is too small, two tables in turn at depth 4 declared new; passes with row
text on, under -c RF and with MCALLER_NARROW_RECORDS=0 take the wide layout and give the same records.  Runs on a real MI355X only."""
import os

import numpy as np
import pytest

from tests import edge_tables as E
from tests import helpers as H
from tests import narrow_records as N

pytestmark = pytest.mark.gpu
K, SKIP = N.K, N.SKIP


@pytest.fixture()
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope='module')
def weights():
    from mcaller_amd import extract_contexts as ec
    _, w, _, soc = ec.submodel_setup(H.load_modelset('r95'), 'A')
    return w, soc


_ORACLE = {}


def case(name, weights, qual_thresh=None):
    """(table, qualities, quality threshold, scored oracle records) of a table of tests/narrow_records.py, made once"""
    key = (name, qual_thresh)
    if key not in _ORACLE:
        table, qual = getattr(N, name + '_table')()
        qt = qual_thresh if qual_thresh is not None else (N.QUAL_THRESH if name == 'crossing' else 0.0)
        orc = H.oracle_records(table, E.ref_of(N.MOTIF).arrays, qual, K, SKIP, qt)
        H.oracle_score(orc, table, qual, weights[0], weights[1], K)
        _ORACLE[key] = (table, qual, qt, orc)
    return _ORACLE[key]


def took_narrow(rec, orc, what):
    """The pass as it arrived: the encoder's columns and run list, the layout's bytes -- then the records, rebuilt."""
    n = orc.n
    assert rec.n == n and rec._narrow is not None and rec._site_pos is None, '%s: not narrow records' % what
    want = N.encode(orc.site_pos[:n], orc.site_seg[:n], orc.info[:n], orc.close_row[:n])
    assert rec.n_runs == len(want[4]) // 4, '%s: %d runs, the reference counts %d' % (what, rec.n_runs, len(want[4]) // 4)
    for name, a, b in zip(('close_lo16', 'pos_lo16', 'info_lo16', 'info_next', 'runs'), rec._narrow, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), '%s: %s differs' % (what, name)
    assert rec.copy_out_bytes == N.narrow_bytes(n, rec.n_calls, K, N.n_wide_of(rec), rec.n_runs), what
    H.assert_records_equal(rec, orc, K, prob_tol=1e-6)


def took_wide(rec, orc, what):
    n = orc.n
    assert rec.n == n and rec._narrow is None and rec.n_runs == 0, '%s: not the wide columns' % what
    assert rec.copy_out_bytes == N.wide_bytes(n, rec.n_calls, K, N.n_wide_of(rec)), what
    H.assert_records_equal(rec, orc, K, prob_tol=1e-6)


def both_ways(dev, weights, name, passes=2):
    table, qual, qt, orc = case(name, weights)
    dev.set_reference(E.ref_of(N.MOTIF).arrays)
    dev.set_mlp(*weights)
    dev.upload_table(table)
    dev.set_read_quality(qual)
    sync = dev.extract(K, SKIP, qt)
    H.assert_records_equal(sync, orc, K, prob_tol=1e-6)
    dev.upload_table_async(table, qual)
    for i in range(passes):                 # (a table's first pass validates it, the later ones stream its summaries)
        dev.run_async(K, SKIP, qt)
        rec = dev.wait()
        assert dev.last_pass_info()[1] == 0, '%s, pass %d was repeated' % (name, i)
        took_narrow(rec, orc, '%s, pass %d' % (name, i))
        H.assert_records_equal(rec, sync, K, prob_tol=1e-6)
    dev.sync()
    return orc


def test_records_on_both_sides_of_row_65536(dev, weights):
    orc = both_ways(dev, weights, 'straddle')
    close = orc.close_row[:orc.n]
    assert close.min() < 65536 < close.max()


def test_sites_across_a_multiple_of_65536_and_a_filtered_read_between(dev, weights):
    orc = both_ways(dev, weights, 'crossing')
    assert sorted(set(orc.site_seg[:orc.n].tolist())) == [0, 2]


def test_reads_of_one_record_each(dev, weights):
    orc = both_ways(dev, weights, 'single_record')
    assert orc.n > N.PACK_WGS


def test_runs_that_start_on_the_edges_of_chunks_and_ranges(dev, weights):
    both_ways(dev, weights, 'mixed')


def test_a_pass_with_no_record(dev, weights):
    table, qual, _, _ = case('crossing', weights)
    dev.set_reference(E.ref_of(N.MOTIF).arrays)
    dev.set_mlp(*weights)
    dev.upload_table_async(table, qual)
    dev.run_async(K, SKIP, 100.0)
    dev.run_async(K, SKIP, N.QUAL_THRESH)
    rec = dev.wait()
    assert rec.n == 0 and rec.n_runs == 0 and rec.copy_out_bytes == 0 and rec.n_calls == 0
    took_narrow(dev.wait(), case('crossing', weights)[3], 'behind the empty pass')
    dev.sync()


def test_a_packed_block_that_is_too_small(dev, weights, monkeypatch):
    """The block is sized from the narrow layout: 100 records' worth does not hold 700; the pass is repeated, the next fits."""
    table, qual, qt, orc = case('single_record', weights)
    dev.set_reference(E.ref_of(N.MOTIF).arrays)
    dev.set_mlp(*weights)
    dev.upload_table_async(table, qual)
    monkeypatch.setenv('MCALLER_PACK_RECORDS', '100')
    dev.run_async(K, SKIP, qt)
    monkeypatch.delenv('MCALLER_PACK_RECORDS')
    dev.run_async(K, SKIP, qt)
    rec = dev.wait()
    assert dev.last_pass_info()[1] == 1
    assert rec.n_runs == 0 and rec._narrow is None
    H.assert_records_equal(rec, orc, K, prob_tol=1e-6)
    rec = dev.wait()
    assert dev.last_pass_info()[1] == 0
    took_narrow(rec, orc, 'behind the repeated pass')
    dev.sync()


def test_two_tables_in_turn_at_depth_four(dev, weights):
    a, b = case('mixed', weights), case('crossing', weights)
    dev.set_reference(E.ref_of(N.MOTIF).arrays)
    dev.set_mlp(*weights)
    slots = [dev.upload_table_async(c[0], c[1]) for c in (a, b)]
    assert slots[0] != slots[1]
    order = [0, 1, 0, 1, 1, 0, 0, 1]
    for start in (0, 4):
        for i in order[start:start + 4]:
            dev.select_table(slots[i], as_new=True)
            dev.run_async(K, SKIP, (a, b)[i][2])
        for i in order[start:start + 4]:
            took_narrow(dev.wait(), (a, b)[i][3], 'table %d in turn' % i)
    dev.sync()


def test_the_wide_columns_on_request(dev, weights, monkeypatch):
    table, qual, qt, orc = case('mixed', weights)
    dev.set_reference(E.ref_of(N.MOTIF).arrays)
    dev.set_mlp(*weights)
    dev.upload_table_async(table, qual)
    monkeypatch.setenv('MCALLER_NARROW_RECORDS', '0')
    dev.run_async(K, SKIP, qt)
    monkeypatch.delenv('MCALLER_NARROW_RECORDS')
    dev.run_async(K, SKIP, qt)
    wide, narrow = dev.wait(), dev.wait()
    sent = wide.copy_out_bytes
    took_wide(wide, orc, 'MCALLER_NARROW_RECORDS=0')
    took_narrow(narrow, orc, 'the pass behind it')
    assert sent - narrow.copy_out_bytes == N.wide_bytes(orc.n, 0, K, 0) - N.narrow_bytes(orc.n, 0, K, 0, narrow.n_runs)
    dev.sync()


def test_a_forest_takes_the_wide_columns(dev, weights):
    from mcaller_amd import extract_contexts as ec
    table, qual, qt, _ = case('mixed', weights)
    _, forests, _, soc = ec.submodel_setup(H.load_rf_modelset(), 'A')
    orc = H.oracle_records(table, E.ref_of(N.MOTIF).arrays, qual, K, SKIP, qt)
    H.oracle_score(orc, table, qual, forests, soc, K)
    dev.set_reference(E.ref_of(N.MOTIF).arrays)
    dev.set_classifier(forests, soc)
    dev.upload_table_async(table, qual)
    for _ in range(2):
        dev.run_async(K, SKIP, qt)
    for i in range(2):
        rec = dev.wait()
        assert rec._narrow is None and rec.n_runs == 0 and rec.copy_out_bytes == N.wide_bytes(orc.n, rec.n_calls, K, N.n_wide_of(rec))
        H.assert_records_equal(rec, orc, K, prob_tol=0.0)
    dev.sync()


def test_a_pass_whose_rows_the_device_writes_takes_the_wide_columns(dev, weights, tmp_path):
    """mc_rowtext.hip reads the packed block on the device: the same records and the host formatter's rows, as before."""
    from mcaller_amd import _lib, synth
    codes = synth.genome(length=400000, seed=5)
    ref = synth.SynthRef(codes)
    table, qual = synth.make_table(60000, seed=3, codes=codes)
    orc = H.oracle_records(table, ref.device_arrays(), qual, K, SKIP, 0.0)
    H.oracle_score(orc, table, qual, weights[0], weights[1], K)
    assert orc.n > 50
    tsv = str(tmp_path / 'rows.eventalign.tsv')
    synth.write_tsv_native(table, codes, tsv)
    dev.set_reference(ref.device_arrays())
    dev.set_mlp(*weights)
    text = _lib.TextBlock(tsv, 0, os.path.getsize(tsv))
    parsed = dev.parse_end(dev.parse_begin(text, ['ecoli_syn'], table.n_rows + 4096), text)
    assert parsed is not None and parsed.n_rows == table.n_rows
    dev.upload_table_async(parsed, np.asarray(qual, dtype=np.float64))
    dev.row_text(True, 'm6A', 'A')
    dev.run_async(K, SKIP, 0.0)
    dev.row_text(False)
    dev.run_async(K, SKIP, 0.0)
    got = dev.wait()
    took_wide(got, orc, 'row text on')
    rows = getattr(got, 'row_text', None)
    assert rows is not None, 'no rows from the device for this pass'
    fmt = _lib.DiffsFormatter(got, parsed, ref.device_arrays(), ref.names, [str(float(q)) for q in qual], K, 'm6A', 'A', weights[1])
    blob, n_rows, stop = fmt.rows(0)
    assert stop >= got.n and n_rows == rows.n_rows and bytes(blob.view) == bytes(rows.view)
    rows.release()
    behind = dev.wait()                       # (row text off again: narrow records, and the formatter prints the same rows from them)
    took_narrow_rows = _lib.DiffsFormatter(behind, parsed, ref.device_arrays(), ref.names, [str(float(q)) for q in qual], K, 'm6A', 'A', weights[1])
    blob2, n_rows2, stop2 = took_narrow_rows.rows(0)
    assert behind._narrow is not None and behind._site_pos is None
    assert stop2 >= behind.n and n_rows2 == n_rows and bytes(blob2.view) == bytes(blob.view)
    took_narrow(behind, orc, 'behind the pass with row text')
    dev.sync()
