"""Narrow records (mc_calls_view.close_lo16, narrow_layout in csrc/mc_dev.h), restated in numpy: the reference encoder and decoder
of the four record columns, the size of a packed block in either layout, and Records objects that hold hand-written columns the
way mc_wait_records hands them out.  Shared by tests/test_narrow_records.py (CPU) and tests/test_gpu_narrow_records.py."""
import functools

import numpy as np

from mcaller_amd import _lib


def run_starts(site_pos, site_seg, close_row):
    """bool [n]: record j starts a run iff j == 0 or (site_seg, close_row >> 16, site_pos >> 16) differs from record j - 1's
    (arithmetic shifts; nothing is assumed about order)."""
    pos, seg, close = (np.asarray(a, dtype=np.int64) for a in (site_pos, site_seg, close_row))
    n = len(pos)
    start = np.ones(n, dtype=bool)
    if n > 1:
        start[1:] = (seg[1:] != seg[:-1]) | ((close[1:] >> 16) != (close[:-1] >> 16)) | ((pos[1:] >> 16) != (pos[:-1] >> 16))
    return start


def encode(site_pos, site_seg, info, close_row):
    """-> (close_lo16, pos_lo16, info_lo16, info_next, runs int32 [n_runs * 4])"""
    pos, seg, close = (np.asarray(a, dtype=np.int64) for a in (site_pos, site_seg, close_row))
    info = np.asarray(info, dtype=np.uint32)
    assert not (info >> 24).any(), 'an info word with a bit in 24..31 does not fit'
    first = np.nonzero(run_starts(pos, seg, close))[0]
    runs = np.stack([first, seg[first], close[first] >> 16, pos[first] >> 16], axis=1).astype(np.int32).reshape(-1) if len(first) else np.zeros(0, dtype=np.int32)
    return ((close & 0xFFFF).astype(np.uint16), (pos & 0xFFFF).astype(np.uint16), (info & 0xFFFF).astype(np.uint16),
            (info >> 16).astype(np.uint8), np.ascontiguousarray(runs))


def decode(close_lo16, pos_lo16, info_lo16, info_next, runs):
    """-> (site_pos int32, site_seg int32, info uint32, close_row int64); any run list that begins at record 0 and ascends"""
    n = len(close_lo16)
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 4)
    info = info_lo16.astype(np.uint32) | (info_next.astype(np.uint32) << 16)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), info, np.zeros(0, np.int64)
    assert runs[0, 0] == 0 and (np.diff(runs[:, 0]) > 0).all() and runs[-1, 0] < n
    of = np.searchsorted(runs[:, 0], np.arange(n), side='right') - 1
    pos = ((runs[of, 3] << 16) | pos_lo16.astype(np.int64)).astype(np.int32)
    close = (runs[of, 2] << 16) | close_lo16.astype(np.int64)
    return pos, runs[of, 1].astype(np.int32), info, close


def tail_bytes(feats_off, m, k, n_wide):
    """pack_tail(...).end: lo32[m * k] | prob[m] | wide mask[m] | hi32[n_wide] behind the record columns"""
    prob = (feats_off + m * k * 4 + 7) & ~7
    hi32 = (prob + m * 8 + m + 3) & ~3
    return hi32 + n_wide * 4


def wide_bytes(n, m, k, n_wide, close32=True):
    """Bytes of a packed block whose record columns travel in full (pack_layout)."""
    return tail_bytes((n * (4 if close32 else 8) + 3 * n * 4 + 7) & ~7, m, k, n_wide)


def narrow_bytes(n, m, k, n_wide, n_runs):
    """... as narrow records (narrow_layout): 7 bytes per record, the run list 16-byte aligned behind them."""
    return tail_bytes(((n * 7 + 15) & ~15) + 16 * n_runs, m, k, n_wide)


def n_wide_of(rec):
    """Wide slot means of a pass as it arrived (nothing unpacked yet)."""
    return len(rec._packed[1]) if rec._packed is not None else 0


def plain(site_pos, site_seg, info, close_row, k=6):
    """Records with one feats / prob row per record over hand-written columns (slot means 0, probability 0.25)."""
    n = len(site_pos)
    r = _lib.Records(n, k)
    r.n = n
    r.site_pos[:n], r.site_seg[:n], r.info[:n], r.close_row[:n] = site_pos, site_seg, info, close_row
    r.prob[:] = 0.25
    return r


def narrowed(rec, runs=None):
    """The same records with their four columns as narrow records (the slot means and probabilities shared); runs: another
    run list for the same columns (a finer one is as valid for a reader)."""
    n = rec.n
    enc = encode(rec.site_pos[:n], rec.site_seg[:n], rec.info[:n], rec.close_row[:n])
    if runs is not None:
        enc = enc[:4] + (np.ascontiguousarray(runs, dtype=np.int32).reshape(-1),)
    c = _lib.Records.__new__(_lib.Records)
    c.k, c.capacity, c.n = rec.k, rec.capacity, n
    c._narrow = enc
    c._feats, c._packed, c.prob = rec._feats, rec._packed, rec.prob
    c._compacted, c._call_row = rec._compacted, rec._call_row
    if rec._compacted:
        c._n_calls = rec._n_calls
    return c


def finest_runs(site_pos, site_seg, close_row):
    """Every record an entry of its own."""
    pos, seg, close = (np.asarray(a, dtype=np.int64) for a in (site_pos, site_seg, close_row))
    return np.stack([np.arange(len(pos)), seg, close >> 16, pos >> 16], axis=1).astype(np.int32).reshape(-1)


# ---------------------------------------------------------------------------------------------------
# the tables of tests/test_gpu_narrow_records.py (tests/test_narrow_records.py holds their claims on the CPU)
# ---------------------------------------------------------------------------------------------------
MOTIF, K, SKIP = 'GATC', 6, 0
LOW_QUAL, QUAL_THRESH = 5.0, 7.0        # (the pools' qualities lie in 6 .. 12: every read but the filtered one gets 8 or more)
PACK_WGS, SIDE_WGS = 512, 128           # MC_PACK_WGS; workgroups of the side kernel under a sparse motif (MC_SIDE_WGS_SPARSE)


def _lay(reads, low=()):
    from tests import edge_tables as E
    t, q = E.table_of(reads)
    q = np.maximum(q, 8.0)
    for i in low:
        q[i] = LOW_QUAL
    return t, q


def _straddle_reads():
    from tests import edge_tables as E
    short, long_ = E.Cursor(E.pool_of('short'), 5), E.Cursor(E.pool_of('long'), 2)
    reads, n = [], 0
    while n < 64000:
        reads.append(short.take())
        n += len(reads[-1])
    while True:
        r = long_.take()
        if n + len(r) > 65536 + 600 and 65536 - n > 600:
            break
    return reads + [r, short.take()]


def straddle_table():
    """A little over 65 536 rows: short reads up to row 64 000 or so, then a long read that holds row 65 536 with records on
    either side of it, then a short one."""
    return _lay(_straddle_reads())


def crossing_table():
    """Three reads: one whose event indices rise ('+') and one whose indices fall ('-'), each with sites on both sides of a
    reference position that is a multiple of 65 536, and between them a read under the quality threshold."""
    from tests import edge_tables as E
    from tests import whole_tile_cases as W
    from tests import helpers as H
    ref, found = E.ref_of(MOTIF), {}
    for r in W.long_pool().reads + E.pool_of('long').reads + E.pool_of('short').reads:
        hi16 = r.pos.astype(np.int64) >> 16
        at = np.nonzero(hi16 != hi16[0])[0]
        if len(at) == 0 or r.up() in found:
            continue
        a = max(0, int(at[0]) - 2500)
        while r.fl[a] & E.N_FLAG:
            a += 1
        piece = r.cut(a, min(len(r), int(at[0]) + 2500))
        t, q = _lay([piece])
        orc = H.oracle_records(t, ref.arrays, q, K, SKIP, 0.0)
        if len(np.unique(orc.site_pos[:orc.n] >> 16)) == 2:           # (records on both sides)
            found[r.up()] = piece
    assert set(found) == {True, False}, 'no read of either strand across a multiple of 65 536'
    return _lay([found[True], E.pool_of('short').reads[7], found[False]], low=(1,))


@functools.lru_cache(maxsize=None)
def _single_reads(count):
    from tests import edge_tables as E
    from tests import helpers as H
    ref = E.ref_of(MOTIF)
    pieces = []
    for r in E.pool_of('short').reads:
        offs = ref.site_off(K)[0 if r.up() else 1]
        rows = [i for i in range(len(r)) if not (r.fl[i] & E.N_FLAG) and offs[int(r.pos[i])] >= 0]
        for z in rows[::4]:
            if z >= 16 and z + 16 <= len(r) and not (r.fl[z - 16] & E.N_FLAG):
                pieces.append(r.cut(z - 16, z + 16))
        if len(pieces) > 3 * count:
            break
    t, q = _lay(pieces)
    orc = H.oracle_records(t, ref.arrays, q, K, SKIP, 0.0)
    per_seg = np.bincount(orc.site_seg[:orc.n], minlength=len(pieces))
    one = [p for p, c in zip(pieces, per_seg) if c == 1][:count]
    assert len(one) == count, 'only %d pieces of one record' % len(one)
    return one


def single_record_table(count=700):
    """`count` reads of one record each (pieces of 32 rows of the short pool's reads around one site row): every record starts
    a run -- and with more than PACK_WGS of them a packing chunk holds two records, both run starts."""
    return _lay(_single_reads(count))


def mixed_table():
    """Between 512 and 1024 records, so that a packing chunk holds two and a workgroup's range eight: reads of one record and
    reads of several, so that runs start on a chunk's first record, on its last, on a range's first and last -- and do not."""
    one = _single_reads(700)
    return _lay(one[:300] + _straddle_reads()[:60] + one[300:560])
