"""Narrow records on the host: the four record columns of a pipelined pass as 16-bit halves plus a run list
(mc_calls_view.close_lo16; written by k2_mlp<.., PACK>, csrc/mc_dev.h narrow_layout).  A numpy encoder and decoder state the
format (tests/narrow_records.py); hand-written columns go through mc_records_expand, mc_calls_expand, mc_count_records and
mc_format_diffs in both layouts and must give the same columns, counts and text.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from mcaller_amd import _lib
from tests import helpers as H
from tests import narrow_records as N



def _cases():
    """name -> (site_pos, site_seg, info, close_row, number of runs)"""
    a = lambda *v: np.array(v, dtype=np.int64)
    c = {}
    c['no record'] = (a(), a(), a(), a(), 0)
    c['one record'] = (a(70000), a(3), a(0x410100), a(65536), 1)
    c['every record its own run'] = (a(5, 9, 13, 17), a(0, 1, 2, 3), a(0, 0x100, 0x200, 0x400), a(10, 20, 30, 40), 4)
    c['one run for all records'] = (a(5, 9, 13, 65535), a(2, 2, 2, 2), a(1, 2, 4, 8), a(10, 20, 30, 65535), 1)
    c['a run that starts at the last record'] = (a(5, 9, 13, 17), a(2, 2, 2, 3), a(0, 0, 0, 0), a(10, 20, 30, 40), 2)
    c['close_row over 65535 -> 65536'] = (a(5, 9, 13), a(0, 0, 0), a(0, 0, 0), a(65534, 65535, 65536), 2)
    c['close_row over two multiples at once'] = (a(5, 9, 13), a(0, 0, 0), a(0, 0, 0), a(65535, 65535 + 2 * 65536, 4 * 65536), 3)
    c['site_pos rising across a multiple'] = (a(65534, 65535, 65536, 65537), a(1, 1, 1, 1), a(0, 0, 0, 0), a(7, 8, 9, 10), 2)
    c['site_pos falling across a multiple'] = (a(131073, 131072, 131071, 131070), a(1, 1, 1, 1), a(0x100, 0x100, 0x100, 0x100), a(7, 8, 9, 10), 2)
    c['site_pos at 0'] = (a(0, 1, 65536, 0), a(4, 4, 4, 4), a(0, 0, 0, 0), a(1, 2, 3, 4), 3)
    c['a negative site_pos'] = (a(-1, 0, -65536, -65537), a(0, 0, 0, 0), a(0, 0, 0, 0), a(1, 2, 3, 4), 4)
    c['a segment change with both high halves equal'] = (a(100, 101, 102), a(6, 6, 7), a(0, 0, 0), a(50, 51, 52), 2)
    c['equal keys separated by a different one'] = (a(100, 70000, 101, 102), a(6, 6, 6, 6), a(0, 0, 0, 0), a(50, 51, 52, 53), 3)
    bits = [1 << b for b in range(16)]
    c['every info bit and the highest context byte'] = (a(*range(200, 217)), a(*([0] * 9 + [1] * 8)), a(*(bits + [0xFFFFFF])),
                                                       a(*range(65530, 65547)), 3)
    c['a closing row of 2^31 - 2'] = (a(9, 10), a(0, 0), a(0, 0), a(2 ** 31 - 3, 2 ** 31 - 2), 1)
    return c


CASES = _cases()


def _columns(case):
    pos, seg, info, close, n_runs = CASES[case]
    return pos.astype(np.int32), seg.astype(np.int32), info.astype(np.uint32), close.astype(np.int64), n_runs


def _expand(rec, n):
    pos, seg, info, close = (np.full(max(1, n), 123, dtype=t) for t in (np.int32, np.int32, np.uint32, np.int64))
    v = rec.view()
    _lib.check(_lib.lib().mc_records_expand(C.byref(v), n, pos.ctypes.data, seg.ctypes.data, info.ctypes.data, close.ctypes.data))
    rows, close2 = np.full(max(1, n), -7, dtype=np.int32), np.full(max(1, n), -7, dtype=np.int64)
    _lib.check(_lib.lib().mc_calls_expand(C.byref(v), n, rec.k, rows.ctypes.data, close2.ctypes.data, None))
    assert np.array_equal(close[:n], close2[:n]) and np.array_equal(rows[:n], np.arange(n))
    return pos[:n], seg[:n], info[:n], close[:n]


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_encoder_the_decoder_and_the_library_agree(case):
    pos, seg, info, close, n_runs = _columns(case)
    n = len(pos)
    enc = N.encode(pos, seg, info, close)
    assert len(enc[4]) == 4 * n_runs and int(N.run_starts(pos, seg, close).sum()) == n_runs
    for a, b in zip(N.decode(*enc), (pos, seg, info, close)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    wide = N.plain(pos, seg, info, close)
    lists = [None] + ([N.finest_runs(pos, seg, close)] if n else [])
    for runs in lists:                                   # (the list as the rule makes it, and the finest one: a reader takes either)
        narrow = N.narrowed(wide, runs)
        v = narrow.view()
        if n:
            assert v.close_lo16 and v.pos_lo16 and v.info_lo16 and v.info_next and v.runs and not v.site_pos and not v.info
            assert v.n_runs == (n_runs if runs is None else n)
        for got, want in zip(_expand(narrow, n), _expand(wide, n)):
            assert np.array_equal(got, want)
        for got, want in zip(_expand(narrow, n), (pos, seg, info, close)):
            assert np.array_equal(got, want)
        # the properties rebuild the columns on first use; the view then hands out the rebuilt ones
        if n:
            assert narrow.end_segments() == (int(seg[0]), int(seg[-1]))
        assert np.array_equal(narrow.site_pos[:n], pos) and np.array_equal(narrow.site_seg[:n], seg)
        assert np.array_equal(narrow.info[:n], info) and np.array_equal(narrow.close_row[:n], close)
        if n:
            v = narrow.view()
            assert v.site_pos and v.site_seg and v.info and v.close_row and not v.close_lo16 and not v.runs


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_counters_of_a_shard_in_both_layouts(case):
    pos, seg, info, close, _ = _columns(case)
    n = len(pos)
    if n == 0:
        return
    seg_read = np.arange(int(seg.max()) + 1, dtype=np.int32)[::-1].copy()
    wide = N.plain(pos, seg, info, close)
    marks = [np.zeros(70000, dtype=np.uint8) for _ in range(3)]
    want = wide.count(n, seg_read=seg_read, pos_marks=marks[0])
    got = N.narrowed(wide).count(n, seg_read=seg_read, pos_marks=marks[1])
    fine = N.narrowed(wide, N.finest_runs(pos, seg, close)).count(n, seg_read=seg_read, pos_marks=marks[2])
    assert got == want and fine == want
    assert np.array_equal(marks[0], marks[1]) and np.array_equal(marks[0], marks[2])
    too = (info & _lib.I_TOO_MANY) != 0
    assert want[0][0] == int(too.sum()) and want[0][2] == int(((info & _lib.I_MULTI) != 0).sum())
    if (~too).any():
        assert want[2] == int(pos[~too].min()) and want[3] == int(pos[~too].max()) + 1


def test_a_run_list_that_is_not_one_is_refused():
    pos, seg, info, close, _ = _columns('equal keys separated by a different one')
    wide = N.plain(pos, seg, info, close)
    good = N.encode(pos, seg, info, close)[4]
    out = np.zeros(len(pos), dtype=np.int32)
    for bad in (good[4:], np.concatenate([good[:4], good[:4]]), np.concatenate([good, [len(pos), 0, 0, 0]]),
                np.concatenate([good[:4], good[8:], good[4:8]])):
        v = N.narrowed(wide, bad).view()
        assert _lib.lib().mc_records_expand(C.byref(v), len(pos), out.ctypes.data, None, None, None) == -12
        assert _lib.lib().mc_count_records(C.byref(v), len(pos), None, 0, None, None, None, 0, None, None) == -12


@pytest.fixture(scope='module')
def shard():
    """A table whose rows and positions pass many multiples of 65 536 (enough records for the formatter to cut them into pieces), its scored oracle records as a pipelined pass hands
    them out (compacted, packed slot means, 32-bit closing rows), and the text of its rows from the wide layout."""
    from mcaller_amd import synth
    from mcaller_amd.extract_contexts import submodel_setup
    from tests.test_host_pipeline import _compacted
    codes = synth.genome(length=400000, seed=5)
    ref = synth.SynthRef(codes)
    table, qual = synth.make_table(2400000, seed=3, codes=codes)
    _, weights, _, soc = submodel_setup(H.load_modelset('r95'), 'A')
    rec = H.oracle_records(table, ref.device_arrays(), qual, 6, 0, 0.0)
    H.oracle_score(rec, table, qual, weights, soc, 6)
    n = rec.n
    starts = np.nonzero(N.run_starts(rec.site_pos[:n], rec.site_seg[:n], rec.close_row[:n]))[0]
    assert n > 4200 and rec.close_row[:n].max() > 2 * 65536 and len(np.unique(rec.site_pos[:n] >> 16)) > 3 and 8 < len(starts) < n // 2

    def formatter(r):
        return _lib.DiffsFormatter(r, table, ref.device_arrays(), ref.names, [str(float(q)) for q in qual], 6, 'm6A', 'A', soc)
    return dict(rec=rec, sent=_compacted(rec, 6, as_sent=True), table=table, starts=starts, formatter=formatter)


def _rows(fmt, first, n, threads):
    """The rows from record `first` on: the formatter stops at a record the host handles itself -- taken up behind it."""
    out, n_rows = [], 0
    while first < n:
        blob, rows, stop = fmt.rows(first, n_threads=threads)
        out.append(bytes(blob.view))
        n_rows += rows
        first = stop + 1
    return b''.join(out), n_rows


def test_the_formatter_prints_the_same_rows_from_both_layouts(shard):
    """... from the first record, from the middle of a run, from a run's first and last record, on one thread and on several;
    for records as the synchronous pass leaves them and as a pipelined pass sends them; with the list the rule makes and the finest."""
    n, starts = shard['rec'].n, shard['starts']
    mid = [int(s) + 1 for s, e in zip(starts[:-1], starts[1:]) if e - s > 2][:2]
    firsts = [0, mid[0], mid[1], int(starts[3]), int(starts[4]) - 1, int(starts[-1]), n - 1, n]
    assert all(f not in starts for f in mid)
    for base in (shard['rec'], shard['sent']):
        wide = shard['formatter'](base)
        fine = N.finest_runs(base.site_pos[:n], base.site_seg[:n], base.close_row[:n])
        for runs in (None, fine):
            narrow = N.narrowed(base, runs)
            v = narrow.view()
            assert v.close_lo16 and not v.site_pos and v.n_runs == (len(starts) if runs is None else n)
            fmt = shard['formatter'](narrow)
            for first in firsts:
                for threads in (1, 3):
                    want, got = _rows(wide, first, n, threads), _rows(fmt, first, n, threads)
                    assert got == want, (first, threads)
                    assert first > 0 or want[1] > 500
            assert narrow._site_pos is None                     # (nothing was rebuilt for the formatter)
            seg_read = shard['table'].seg_read
            assert narrow.count(n, seg_read=seg_read) == base.count(n, seg_read=seg_read)
            assert narrow._site_pos is None


def test_the_row_writer_leaves_narrow_records_as_they_arrived(shard):
    """rows.py binds a shard's records without reading their columns: a shard printed by the native formatter and counted by
    mc_count_records rebuilds nothing; by_record() and the per-record path rebuild them once, the oracle's."""
    rec, n = shard['rec'], shard['rec'].n
    narrow = N.narrowed(shard['sent'])
    back = narrow.by_record()
    for name in ('site_pos', 'site_seg', 'info', 'close_row'):
        assert np.array_equal(getattr(back, name)[:n], getattr(rec, name)[:n]), name
    assert np.array_equal(back.feats[:n * 6].view(np.uint64), rec.feats[:n * 6].view(np.uint64))
    assert narrow.n_runs == len(shard['starts']) and narrow._site_pos is not None


def test_the_tables_of_the_gpu_tests_hold_what_they_claim():
    """tests/test_gpu_narrow_records.py runs these on the device; what makes each of them a case is said here, from the oracle."""
    from tests import edge_tables as E
    arrays = E.ref_of(N.MOTIF).arrays

    def of(table_qual, qual_thresh=0.0):
        t, q = table_qual
        o = H.oracle_records(t, arrays, q, N.K, N.SKIP, qual_thresh)
        n = o.n
        assert not (o.info[:n] >> 24).any()
        return t, o.site_pos[:n].astype(np.int64), o.site_seg[:n], o.close_row[:n], (o.info[:n] & _lib.I_REV) != 0, N.run_starts(o.site_pos[:n], o.site_seg[:n], o.close_row[:n])

    t, pos, seg, close, rev, start = of(N.straddle_table())
    assert 65536 < t.n_rows < 80000
    inside = seg[1:] == seg[:-1]
    assert (inside & ((close[1:] >> 16) != (close[:-1] >> 16))).any()          # a run begins inside a read because the closing rows pass 65 536
    t, pos, seg, close, rev, start = of(N.crossing_table(), N.QUAL_THRESH)
    assert t.n_seg == 3 and sorted(set(seg.tolist())) == [0, 2]                 # the read in the middle is filtered
    inside = (seg[1:] == seg[:-1]) & ((pos[1:] >> 16) != (pos[:-1] >> 16))
    assert (inside & ~rev[1:]).any() and (inside & rev[1:]).any()               # '+' and '-'
    assert of(N.crossing_table(), 100.0)[1].size == 0                           # ... and all three are: a pass with no record
    t, pos, seg, close, rev, start = of(N.single_record_table())
    assert len(pos) == t.n_seg > N.PACK_WGS and start.all()
    t, pos, seg, close, rev, start = of(N.mixed_table())
    n = len(pos)
    per = -(-n // N.PACK_WGS)
    assert per == 2 and N.PACK_WGS % N.SIDE_WGS == 0
    span = per * N.PACK_WGS // N.SIDE_WGS                                        # records of a workgroup's range
    j = np.arange(n)
    for every, at in ((per, 0), (per, per - 1), (span, 0), (span, span - 1)):
        here = j % every == at
        assert start[here].any() and (~start[here]).any(), (every, at)
