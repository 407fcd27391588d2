"""The per-site reduction on the device -- k_site_fill, k_site_counts, k_site_status_out and the mc_site_counts* calls of
mc_stream.hip, mc_site_allreduce (no communicator) of mc_comm.hip -- on the cases of tests/site_cases.py: exact integer equality
with the plain restatement of the C oracle's records, for the numbering under every reference setter, every way a pass can run,
the label rule at p = 0.5, contig seams and the table's tail, the streamed life cycle of a sharded file, the host's additions
and the error paths.  `first` is compared where a site has records and must be INT64_MAX elsewhere; every reduction also checks
the number of records left to the host and of cross-contig records it reports.  That the cases hold what they claim is
tests/test_site_cases.py's business (CPU).  Runs on a real MI355X only."""
import numpy as np
import pytest

from mcaller_amd import _lib, make_bed
from tests import site_cases as S

pytestmark = pytest.mark.gpu
PASSES_IN_FLIGHT = 6        # MC_PASSES_IN_FLIGHT: the record sets pipelined passes take turns with


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    return S.cases(str(tmp_path_factory.mktemp('site_cases')))


@pytest.fixture()
def dev():
    """(a context of its own per test: the counts, the status words and the record buffers live in it)"""
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def prepare(dev, case, model=None):
    case.set_reference(dev)
    if model is None:
        dev.set_mlp(*S.weights())
    else:
        dev.set_classifier(*model)


def assert_counts(got, want, how):
    n_meth, n_total, first = got[:3]
    assert len(n_meth) == len(n_total) == len(first) == want.n_sites, how
    for name, a, b in (('n_total', n_total, want.n_total), ('n_meth', n_meth, want.n_meth)):
        if not np.array_equal(a, b):
            s = int(np.flatnonzero(a != b)[0])
            raise AssertionError('%s: %s of site %d is %d, expected %d (%d sites differ)' % (how, name, s, a[s], b[s], int((a != b).sum())))
    seen = want.n_total > 0
    if not np.array_equal(first[seen], want.first[seen]):
        s = int(np.flatnonzero(seen & (first != want.first))[0])
        raise AssertionError('%s: first row of site %d is %d, expected %d' % (how, s, first[s], want.first[s]))
    assert (first[~seen] == S.INT64_MAX).all(), '%s: a site without records has a first row' % how


def same_records(rec, case, tail, model, how):
    """The device's records are the oracle's, one for one (what every probability and every skip mask below is indexed by)."""
    orc = case.records(tail, model)[0]
    r = rec.by_record()
    assert r.n == orc.n, '%s: %d records, the oracle has %d' % (how, r.n, orc.n)
    for name in ('site_pos', 'site_seg', 'close_row', 'info'):
        assert np.array_equal(getattr(r, name)[:r.n], getattr(orc, name)[:r.n]), '%s: %s differs from the oracle' % (how, name)


def fold(dev, case, rec, tail, row_offset, model=None):
    """The records the device left to the host, added the way multi_gpu's worker adds them (make_bed.add_pending_site_counts)."""
    _, prob, _ = case.records(tail, model)
    x = case.expected(tail=tail, row_offset=row_offset, model=model)
    skip = np.zeros(len(prob), dtype=bool)
    skip[x.cross] = True
    index = make_bed.SiteIndex(case.ref.meth, case.n_contigs)
    return make_bed.add_pending_site_counts(dev, rec, case.table, index, row_offset=row_offset, prob=prob, skip=skip)


def reduce_and_check(dev, case, rec, how, tail=None, row_offset=0, model=None, accumulate=False, onto=None):
    """One reduction of the pass handed out last: what it reports, the device's own counts, the counts with the host's records
    added.  accumulate: onto what the context holds (`onto`: the restatement of that) instead of from zero."""
    tail = case.tail if tail is None else tail
    same_records(rec, case, tail, model, how)
    own = case.expected(tail=tail, row_offset=row_offset, model=model, device_only=True)
    want = case.expected(tail=tail, row_offset=row_offset, model=model)
    pending = (dev.site_counts_accumulate if accumulate else dev.site_counts)(row_offset=row_offset, tail_contig=tail)
    assert pending == want.pending, '%s: %d records left to the host, expected %d' % (how, pending, want.pending)
    assert dev.n_cross_contig == want.n_cross, '%s: %d cross-contig records, expected %d' % (how, dev.n_cross_contig, want.n_cross)
    assert_counts(dev.site_counts_fetch(), own if onto is None else S.add(onto, own), how + ', the device alone')
    assert fold(dev, case, rec, tail, row_offset, model) == want.pending
    total = want if onto is None else S.add(onto, want)
    assert_counts(dev.site_counts_fetch(), total, how)
    return total


def run_sync(dev, case, tail=None):
    return dev.extract(case.k, case.skip, 0.0, tail_contig=case.tail if tail is None else tail)


def run_pipelined(dev, case, tail=None):
    dev.run_async(case.k, case.skip, 0.0, tail_contig=case.tail if tail is None else tail)
    return dev.wait()


def upload(dev, case):
    dev.upload_table(case.table)
    dev.set_read_quality(case.qual)


# ---- the numbering ----
@pytest.mark.parametrize('name', ['placed', 'motif', 'iupac'])
def test_numbering_under_every_reference_setter(dev, cases, name):
    """Host-made masks with sites on bits 0, 31, 32, 63, 64, contig seams and both strands (set_reference); masks, rank arrays and
    site_base made on the device (set_reference_motif, set_reference_iupac): the totals are the restatement's, with the
    host-scored edge records added."""
    case = cases[name]
    assert case.setter == {'placed': 'masks', 'motif': 'motif', 'iupac': 'iupac'}[name]
    prepare(dev, case)
    upload(dev, case)
    want = reduce_and_check(dev, case, run_sync(dev, case), name)
    assert want.n_total.sum() > 50 and (name == 'motif' or want.pending > 0)


# ---- the ways a pass can run ----
def test_synchronous_and_pipelined_passes_count_alike(dev, cases):
    """run / extract, then run_async + wait as scan + emit, over the same table: the same counts; and a small table behind the
    larger one, both ways: the slots beyond its records still hold the larger pass's and are not counted."""
    placed, small = cases['placed'], cases['small']
    prepare(dev, placed)
    upload(dev, placed)
    a = reduce_and_check(dev, placed, run_sync(dev, placed), 'synchronous')
    rec = run_pipelined(dev, placed)
    assert dev.last_pass_info() == (0, False)
    b = reduce_and_check(dev, placed, rec, 'pipelined, scan + emit', row_offset=0)
    assert np.array_equal(a.n_total, b.n_total) and np.array_equal(a.n_meth, b.n_meth) and np.array_equal(a.first, b.first)
    upload(dev, small)
    for again in range(PASSES_IN_FLIGHT):           # (until the pass takes the record set the larger one had)
        rec = run_pipelined(dev, small)
        assert dev.last_pass_info() == (0, False)
        reduce_and_check(dev, small, rec, 'a small table behind a larger one, pipelined pass %d' % again)
    upload(dev, placed)
    reduce_and_check(dev, placed, run_sync(dev, placed), 'synchronous again')
    upload(dev, small)
    reduce_and_check(dev, small, run_sync(dev, small), 'a small table behind a larger one, synchronous')


def test_fused_dense_pass(dev, cases):
    """A one-base motif, pipelined: the pass runs as k1_fused (asked of the library), its records lie in per-piece rooms with
    holes between them, and every slot is reduced."""
    dense = cases['dense']
    prepare(dev, dense)
    upload(dev, dense)
    reduce_and_check(dev, dense, run_sync(dev, dense), 'dense, synchronous')
    rec = run_pipelined(dev, dense)
    room, rerun = dev.last_pass_info()
    assert room > 0 and not rerun, 'the pass did not run as the fused kernel (room %d, repeated %r)' % (room, rerun)
    reduce_and_check(dev, dense, rec, 'dense, k1_fused', row_offset=S.BIG_OFFSET)


def test_pass_repeated_inside_wait_and_merged(dev, cases):
    """A read whose position steps back: the pipelined pass is repeated inside wait(), the literal path's records are merged
    with the fast path's (k_merge) and the merged buffer is what is reduced."""
    case = cases['irregular']
    prepare(dev, case)
    upload(dev, case)
    rec = run_pipelined(dev, case)
    assert dev.last_pass_info()[1], 'the pass was not repeated'
    reduce_and_check(dev, case, rec, 'irregular, repeated inside wait', row_offset=1000)
    reduce_and_check(dev, case, run_sync(dev, case), 'irregular, synchronous')


# ---- the label rule ----
@pytest.mark.parametrize('intercept', [0.0, -1e-9])
def test_label_rule_at_one_half(dev, cases, intercept):
    """A logistic model with all-zero coefficients: p is exactly 0.5 for every record the device scores and every one of them
    counts as methylated (the reference's `>= 0.5`); with the intercept at -1e-9 none does."""
    from tests import clf_cases
    from mcaller_amd.model_io import LogisticWeights
    case = cases['placed']
    w, soc = S.weights()
    model = ([LogisticWeights(np.zeros(case.k + 1), intercept, clf_cases.CLASSES) for _ in w], soc)
    _, prob, nan = case.records(model=model)
    assert (prob[~nan] == 0.5).all() if intercept == 0.0 else ((prob[~nan] < 0.5) & (prob[~nan] > 0.5 - 1e-9)).all()
    prepare(dev, case, model)
    upload(dev, case)
    rec = run_sync(dev, case)
    assert dev.site_counts(tail_contig=case.tail) == case.expected(model=model).pending
    n_meth, n_total, _ = dev.site_counts_fetch()
    assert n_total.sum() > 300 and np.array_equal(n_meth, n_total if intercept == 0.0 else np.zeros_like(n_total))
    reduce_and_check(dev, case, rec, 'logistic model, intercept %r' % intercept, model=model)


# ---- contigs and the tail ----
@pytest.mark.parametrize('row_offset', [0, S.BIG_OFFSET])
def test_cross_contig_records_and_the_tail(dev, cases, row_offset):
    """The table ends in an open window: with the site's own contig behind it the record counts and its row is n_rows +
    row_offset, with another contig it is a cross-contig record, with none there is no record; `first` keeps all 64 bits of a
    row offset of a rank far down a sharded file."""
    prepare(dev, cases['placed'])
    for name in ('placed', 'tail only'):
        case = cases[name]
        upload(dev, case)
        for tail in (S.C_LONG, S.C_EMPTY, -1):
            how = '%s, tail_contig %d, row_offset %d' % (name, tail, row_offset)
            want = reduce_and_check(dev, case, run_sync(dev, case, tail), how, tail=tail, row_offset=row_offset)
            if name == 'tail only':
                site = want.number[(S.C_LONG, 1, 394)]
                assert want.n_total.sum() == (1 if tail == S.C_LONG else 0) and want.n_cross == (1 if tail == S.C_EMPTY else 0)
                assert tail != S.C_LONG or want.first[site] == case.table.n_rows + row_offset
            rec = run_pipelined(dev, case, tail)
            reduce_and_check(dev, case, rec, how + ', pipelined', tail=tail, row_offset=row_offset)


# ---- the streamed life cycle ----
def zero(n):
    x = S.Expected()
    x.n_sites, x.n_meth, x.n_total, x.first = n, np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, S.INT64_MAX, np.int64)
    return x


def test_shards_accumulate(dev, cases):
    """reset, three shards with descending row offsets: the counts add up and `first` is the minimum whatever the order; what a
    call reports is that call's alone; the same pass twice doubles its counts; a pass without records changes nothing; reset
    zeroes."""
    prepare(dev, cases['placed'])
    n = cases['placed'].expected().n_sites
    dev.site_counts_reset()
    assert_counts(dev.site_counts_fetch(), zero(n), 'after reset')
    total = zero(n)
    for name, row_offset in (('placed', 2 << 40), ('B', 1 << 40), ('A', 7)):
        case = cases[name]
        dev.upload_table_async(case.table, case.qual)
        rec = run_pipelined(dev, case)
        total = reduce_and_check(dev, case, rec, 'shard %s' % name, row_offset=row_offset, accumulate=True, onto=total)
    a = cases['A']
    assert (total.first[a.expected().n_total > 0] < (1 << 40)).all() and (total.first[total.n_total > 0] >= 7).all()
    # the same pass again: its counts twice, `first` as it was
    total = reduce_and_check(dev, a, rec, 'shard A again', row_offset=7, accumulate=True, onto=total)
    # a pass without a record
    empty = cases['tail only']
    dev.upload_table_async(empty.table, empty.qual)
    rec = run_pipelined(dev, empty, tail=-1)
    assert rec.n == 0
    reduce_and_check(dev, empty, rec, 'a shard without records', tail=-1, row_offset=5, accumulate=True, onto=total)
    dev.site_counts_reset()
    assert_counts(dev.site_counts_fetch(), zero(n), 'after the second reset')


@pytest.mark.parametrize('first_table', ['A', 'A irregular'])
def test_two_tables_in_flight(dev, cases, first_table):
    """Tables A and B, whose segments map to different contigs, both in flight: A's records are reduced on A's table while B is
    the current one -- also when A's pass is repeated inside wait() on its own table."""
    a, b = cases[first_table], cases['B']
    prepare(dev, a)
    dev.site_counts_reset()
    for case in (a, b):
        dev.upload_table_async(case.table, case.qual)
        dev.run_async(case.k, case.skip, 0.0, tail_contig=case.tail)
    rec = dev.wait()
    assert dev.last_pass_info()[1] == (first_table == 'A irregular')
    total = reduce_and_check(dev, a, rec, 'table %s while B is current' % first_table, row_offset=1 << 33, accumulate=True, onto=zero(a.expected().n_sites))
    rec = dev.wait()
    assert not dev.last_pass_info()[1]
    total = reduce_and_check(dev, b, rec, 'table B', row_offset=0, accumulate=True, onto=total)
    assert_counts(dev.site_counts_fetch(), S.add(a.expected(row_offset=1 << 33), b.expected()), 'A + B')


# ---- the host's additions ----
def test_site_counts_add(dev, cases):
    """Records the host scored: the smaller first row wins, whether it is the new one or the one that was there; a site number
    out of range raises the library's error and leaves the counts as they were (the host's copy is discarded)."""
    case = cases['placed']
    prepare(dev, case)
    upload(dev, case)
    want = reduce_and_check(dev, case, run_sync(dev, case), 'placed')
    s = want.number[S.CROWDED]
    f = int(want.first[s])
    dev.site_counts_add([s], [1], [f - 5])
    want.n_total[s] += 1; want.n_meth[s] += 1; want.first[s] = f - 5
    assert_counts(dev.site_counts_fetch(), want, 'a smaller first row')
    dev.site_counts_add([s, s], [0, 1], [f + 100, S.INT64_MAX])
    want.n_total[s] += 2; want.n_meth[s] += 1
    assert_counts(dev.site_counts_fetch(), want, 'a larger first row')
    never = want.number[S.NEVER]
    dev.site_counts_add([never], [0], [S.BIG_OFFSET + 1])
    want.n_total[never] += 1; want.first[never] = S.BIG_OFFSET + 1
    assert_counts(dev.site_counts_fetch(), want, 'a site without records so far')
    for bad in (want.n_sites, -1, 1 << 40):
        with pytest.raises(_lib.McError, match='out of range'):
            dev.site_counts_add([s, bad], [1, 1], [0, 0])
        assert_counts(dev.site_counts_fetch(), want, 'after site %d was refused' % bad)


# ---- errors, another reference, no site at all ----
def test_errors_and_a_new_reference(dev, cases):
    placed, motif = cases['placed'], cases['motif']
    prepare(dev, placed)
    upload(dev, placed)
    rec = run_sync(dev, placed)
    with pytest.raises(_lib.McError, match='call mc_site_counts_reset first'):
        dev.site_counts_accumulate()
    reduce_and_check(dev, placed, rec, 'placed')
    # the same contigs, two sites more: the counts of the old numbering are gone with it
    arrays = dict(placed.ref.device_arrays())
    arrays['mbits_fwd'] = arrays['mbits_fwd'].copy()
    meth = {c: list(m) for c, m in placed.ref.meth.items()}
    for contig, pos in ((S.C_TINY, 0), (S.C_EMPTY, 33)):
        arrays['mbits_fwd'][int(arrays['word_off'][contig]) + pos // 32] |= np.uint32(1 << (pos % 32))
        meth[contig][0] = meth[contig][0][:pos] + 'M' + meth[contig][0][pos + 1:]
    dev.set_reference(arrays)
    with pytest.raises(_lib.McError, match='call mc_site_counts_reset first'):
        dev.site_counts_accumulate()
    # site_counts resets: the records of the last pass under the new numbering, arrays of the new length
    want = placed.expected(meth=meth, device_only=True)
    assert want.n_sites == placed.expected().n_sites + 2
    assert dev.site_counts(tail_contig=placed.tail) == want.pending
    assert_counts(dev.site_counts_fetch(), want, 'two sites more')
    # the same contigs, other sites: a record names a position that is no site; nothing is read out of range, and the next
    # reduction does not inherit the count of such records
    dev.set_reference(motif.ref.device_arrays())
    with pytest.raises(_lib.McError, match='not a marked site'):
        dev.site_counts(tail_contig=placed.tail)
    dev.set_reference(placed.ref.device_arrays())
    assert dev.site_counts(tail_contig=placed.tail) == placed.expected().pending
    assert_counts(dev.site_counts_fetch(), placed.expected(device_only=True), 'the first reference again')


def test_a_reference_without_a_site(dev, cases):
    arrays = dict(cases['placed'].ref.device_arrays())
    arrays['mbits_fwd'], arrays['mbits_rev'] = np.zeros_like(arrays['mbits_fwd']), np.zeros_like(arrays['mbits_rev'])
    dev.set_reference(arrays)
    dev.site_counts_reset()
    assert dev.site_counts_accumulate() == 0 and dev.n_cross_contig == 0
    for got in (dev.site_counts_fetch(), dev.site_allreduce()):
        assert [len(a) for a in got[:3]] == [0, 0, 0] and [a.dtype for a in got[:3]] == [np.int32, np.int32, np.int64]


def test_allreduce_without_a_communicator_is_the_fetch(dev, cases):
    case = cases['placed']
    prepare(dev, case)
    upload(dev, case)
    reduce_and_check(dev, case, run_sync(dev, case), 'placed', row_offset=S.BIG_OFFSET)
    own = dev.site_counts_fetch()
    n_meth, n_total, first, ms = dev.site_allreduce()
    assert ms == 0.0
    for a, b in zip((n_meth, n_total, first), own):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
