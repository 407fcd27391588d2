"""tests/site_cases.py held to its claims, on the CPU: every named placement is a marked site of its case that the C oracle's
records hit the way the builder says; make_bed's numpy reduction (what the host sum of a sharded run relies on) equals the
plain restatement on every case; the BED written from the restated counts equals make_bed's on the .diffs text of the same
records; and no record's probability lies so near 0.5 that the device's classifier could label it differently."""
import contextlib
import io

import numpy as np
import pytest

from mcaller_amd import _lib, make_bed
from tests import site_cases as S


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    return S.cases(str(tmp_path_factory.mktemp('site_cases')))


def records_of(case, contig, rev, pos, tail=None):
    """Indices of the oracle's records that name the site (MC_I_TOO_MANY ones included)."""
    rec, _, _ = case.records(tail)
    return [j for j in range(rec.n) if int(case.table.seg_contig[int(rec.site_seg[j])]) == contig and int(rec.site_pos[j]) == pos and
            bool(int(rec.info[j]) & _lib.I_REV) == bool(rev)]


def mask_bit(case, contig, rev, pos):
    a = case.ref.device_arrays()
    word = int(a['mbits_rev' if rev else 'mbits_fwd'][int(a['word_off'][contig]) + pos // 32])
    return (word >> (pos % 32)) & 1


def test_the_contigs_are_the_lengths_that_were_asked_for(cases):
    placed = cases['placed']
    assert placed.lengths[:8] == [31, 32, 33, 4, 64, 40, 65, 400] and placed.lengths[S.C_TINY] < placed.k
    x = placed.expected()
    per = {(c, s): sum(1 for (cc, ss, _) in x.number if (cc, ss) == (c, s)) for c in range(placed.n_contigs) for s in (0, 1)}
    # a contig shorter than k has sites (they shift the numbers of every contig behind it) and no rows
    assert per[(S.C_TINY, 0)] == 1 and per[(S.C_TINY, 1)] == 1 and not (placed.table.seg_contig == S.C_TINY).any()
    # no site on one strand
    assert per[(S.C_LEN33, 0)] > 0 and per[(S.C_LEN33, 1)] == 0
    # no site at all between two contigs that have some: two equal consecutive entries of site_base, and rows lie on it
    assert per[(S.C_EMPTY, 0)] == per[(S.C_EMPTY, 1)] == 0 and per[(S.C_LEN64, 1)] > 0 and per[(S.C_LEN65, 0)] > 0
    assert (placed.table.seg_contig == S.C_EMPTY).sum() >= 2
    base, n = [], 0
    for c in range(placed.n_contigs):
        for s in (0, 1):
            base.append(n)
            n += per[(c, s)]
    assert base[2 * S.C_EMPTY] == base[2 * S.C_EMPTY + 1] == base[2 * S.C_LEN65] and n == x.n_sites
    # the motif and IUPAC markings find nothing on it either
    for name in ('motif', 'iupac'):
        assert 'M' not in cases[name].ref.meth[S.C_EMPTY][0] + cases[name].ref.meth[S.C_EMPTY][1]


@pytest.mark.parametrize('placement', S.PLACEMENTS, ids=[p[0] for p in S.PLACEMENTS])
def test_every_named_placement_is_hit(cases, placement):
    _, contig, rev, pos, bit, edge = placement
    placed = cases['placed']
    rec, prob, nan = placed.records()
    x = placed.expected()
    assert pos == bit and mask_bit(placed, contig, rev, pos) == 1 and placed.marked(contig, rev, pos)
    hits = [j for j in records_of(placed, contig, rev, pos) if not int(rec.info[j]) & _lib.I_TOO_MANY and j not in x.cross]
    assert hits and x.counted[(contig, rev, pos)][1] == len(hits) == x.n_total[x.number[(contig, rev, pos)]]
    for j in hits:
        assert bool(int(rec.info[j]) & _lib.I_EDGE) == edge and bool(nan[j]) == edge      # (within k of an end: left to the host)
    L, k = placed.lengths[contig], placed.k
    assert edge == (pos - k + 1 < 0 or pos + k > L)
    if placement[0].startswith('L - k of'):
        assert pos == L - k


def test_bit_zero_is_numbered_and_never_counted(cases):
    placed = cases['placed']
    x = placed.expected()
    for contig, rev, pos in S.UNFLUSHED:
        assert pos == 0 and mask_bit(placed, contig, rev, 0) == 1 and not records_of(placed, contig, rev, 0)
        later = [key for key in x.counted if key[:2] == (contig, rev)]
        assert later and all(x.number[key] > x.number[(contig, rev, 0)] for key in later)


def test_both_strands_at_one_position(cases):
    placed = cases['placed']
    x = placed.expected()
    for contig, pos in S.BOTH:
        assert placed.ref.records[contig][1][pos] == 'M'
        a, b = x.number[(contig, 0, pos)], x.number[(contig, 1, pos)]
        assert a != b and x.n_total[a] > 0 and x.n_total[b] > 0


def test_neighbours_in_the_numbering_across_a_contig_seam(cases):
    x = cases['placed'].expected()
    for last, first in S.SEAMS:
        assert x.number[first] == x.number[last] + 1 and last[0] < first[0]
        assert x.n_total[x.number[last]] > 0 and x.n_total[x.number[first]] > 0


def test_crowded_single_and_empty_sites(cases):
    placed = cases['placed']
    x = placed.expected()
    assert x.n_total[x.number[S.CROWDED]] >= S.CROWD and 0 < x.n_meth[x.number[S.CROWDED]] < x.n_total[x.number[S.CROWDED]]
    rows = sorted(int(placed.records()[0].close_row[j]) for j in records_of(placed, *S.CROWDED))
    assert x.first[x.number[S.CROWDED]] == rows[0] and rows[-1] - rows[0] > 2048         # (records of many workgroups)
    assert x.n_total[x.number[S.ONCE]] == 1
    assert placed.marked(*S.NEVER) and x.n_total[x.number[S.NEVER]] == 0 and x.first[x.number[S.NEVER]] == S.INT64_MAX


def test_the_named_cross_contig_record(cases):
    placed = cases['placed']
    contig, rev, pos, closer = S.NAMED_CROSS
    rec, _, nan = placed.records()
    x = placed.expected()
    mine = [j for j in records_of(placed, contig, rev, pos) if j in x.cross]
    assert len(mine) == 1 and not nan[mine[0]]
    row = int(rec.close_row[mine[0]])
    seg = int(np.searchsorted(placed.table.seg_row_begin, row, side='right')) - 1
    assert row == int(placed.table.seg_row_begin[seg]) and placed.ref.names[int(placed.table.seg_contig[seg])] == closer
    assert x.extras[x.cross.index(mine[0])][:3] == (closer, pos, '-' if rev else '+')
    assert x.n_cross == len(x.cross) >= 2 and x.counted[(contig, rev, pos)][1] == len(records_of(placed, contig, rev, pos)) - 1


def test_the_open_window_at_the_end_of_the_table(cases):
    placed = cases['placed']
    site = (S.C_LONG, 1, 394)
    n_rows = placed.table.n_rows
    same, other, nobody = (placed.expected(tail=t, row_offset=S.BIG_OFFSET) for t in (S.C_LONG, S.C_EMPTY, -1))
    assert placed.records(-1)[0].n + 1 == placed.records(S.C_LONG)[0].n == placed.records(S.C_EMPTY)[0].n
    assert int(placed.records(S.C_LONG)[0].close_row[placed.records(S.C_LONG)[0].n - 1]) == n_rows
    assert same.counted[site][1] == nobody.counted[site][1] + 1 == other.counted[site][1] + 1
    assert other.n_cross == same.n_cross + 1 == nobody.n_cross + 1
    assert other.extras[-1][0] == 'empty' and other.extras[-1][5] == n_rows + S.BIG_OFFSET
    # its closing row is the table's row count: the largest of the site, so it is no site's first row here
    assert same.first[same.number[site]] == nobody.first[nobody.number[site]] < n_rows + S.BIG_OFFSET
    # ... and it is the first row of a site in a table of one read
    small = cases['tail only']
    x = small.expected(tail=S.C_LONG, row_offset=S.BIG_OFFSET)
    assert x.counted == {site: [x.counted[site][0], 1, small.table.n_rows + S.BIG_OFFSET]}
    assert small.expected(tail=S.C_EMPTY).n_cross == 1 and small.expected(tail=-1).n_total.sum() == 0


def test_the_irregular_read_and_the_gap(cases):
    for name, want in (('placed', 0), ('irregular', 1), ('A', 0), ('A irregular', 1), ('B', 0)):
        t = cases[name].table
        back = 0
        for s in range(t.n_seg):
            p = t.pos[int(t.seg_row_begin[s]):int(t.seg_row_begin[s + 1])]
            back += int((np.diff(p) < 0).sum())
        assert back == want, name
    # ... and no read of the tables that are to run on the fast path lies on a marked position 0 (it would take the literal path)
    for name in ('placed', 'small', 'A', 'B', 'dense', 'tail only'):
        case = cases[name]
        for s in range(case.table.n_seg):
            c, r = int(case.table.seg_contig[s]), int(case.table.seg_row_begin[s])
            assert case.table.pos[r] > 0 or not (case.marked(c, 0, 0) or case.marked(c, 1, 0)), name
    placed = cases['placed']
    rec, _, _ = placed.records()
    x = placed.expected()
    for pos in (127, 128):
        too = [j for j in records_of(placed, S.C_LONG, 0, pos) if int(rec.info[j]) & _lib.I_TOO_MANY]
        assert len(too) == 1 and x.counted[(S.C_LONG, 0, pos)][1] == len(records_of(placed, S.C_LONG, 0, pos)) - 1 > 0
    # the irregular read's records are counted like any other's
    assert cases['irregular'].expected().n_total.sum() > x.n_total.sum()
    assert cases['A irregular'].expected().n_total.sum() > cases['A'].expected().n_total.sum()


def test_tables_a_and_b_map_their_segments_differently(cases):
    a, b = cases['A'], cases['B']
    right, wrong = a.expected(), a.expected(table=b.table)
    assert right.n_cross != wrong.n_cross and (right.n_total != wrong.n_total).any() and wrong.unmarked == 0
    assert b.table.n_seg >= cases['A irregular'].table.n_seg          # (a record of A indexes B's segments in range)
    assert a.expected().n_total.sum() > 0 and b.expected().n_total.sum() > 0 and (a.expected().n_total != b.expected().n_total).any()


def test_the_dense_case_is_a_dense_reference(cases):
    dense = cases['dense']
    x = dense.expected()
    for name in ('placed', 'motif', 'iupac'):           # (and the others are not: more than 64 bases a site)
        assert (cases[name].expected().n_sites + 2) * 64 <= sum(cases[name].lengths), name
    assert x.n_sites * 64 > sum(dense.lengths) and 8000 < dense.table.n_rows <= 24000 and x.pending > 0
    # the small table run behind a larger one has fewer records than the larger one has slots
    assert 0 < cases['small'].records()[0].n < cases['placed'].records()[0].n


def test_the_three_markings_differ(cases):
    numbers = [set(cases[name].expected().number) for name in ('placed', 'motif', 'iupac')]
    assert numbers[1] < numbers[2] and numbers[0] != numbers[1] and not numbers[0] >= numbers[2]
    assert cases['motif'].ref.motif_for_the_device() is not None and cases['iupac'].ref.iupac_for_the_device() is not None
    assert cases['iupac'].expected().pending > 0 and cases['placed'].expected().pending >= 8
    # device-made masks: sites on bits 31 and 32 of a contig, on both strands, and at L - k
    m = cases['motif'].expected()
    for key in ((S.C_LEN64, 0, 31), (S.C_LEN64, 1, 32), (S.C_LEN65, 0, 31), (S.C_LEN65, 1, 32), (S.C_LONG, 0, 63), (S.C_LONG, 1, 64), (S.C_LONG, 1, 394)):
        assert m.n_total[m.number[key]] > 0, key


def test_no_probability_lies_near_one_half(cases):
    for name, case in cases.items():
        for tail in (case.tail, -1):
            rec, prob, nan = case.records(tail)
            assert (rec.n > 0 or (name, tail) == ('tail only', -1)) and (np.abs(prob[~nan] - 0.5) > 1e-6).all(), name


def host_reduction(case, tail, row_offset):
    """make_bed's numpy reduction of the oracle's records, the way a worker of a sharded run calls it."""
    rec, prob, nan = case.records(tail)
    host_scored = {int(j): float(prob[j]) for j in np.flatnonzero(nan)}
    extras = make_bed.cross_contig_records(rec, case.table, case.ref, case.k, host_scored, case.ref.names[tail] if tail >= 0 else None,
                                           row_offset=row_offset)
    index = make_bed.SiteIndex(case.ref.meth, case.n_contigs)
    return make_bed.site_counts(rec, case.table, index, row_offset=row_offset, prob=prob, skip=extras['records']), extras, index


def test_the_numpy_reduction_equals_the_restatement(cases):
    for name, case in cases.items():
        for tail, row_offset in ((case.tail, 0), (-1, 1000), (S.C_EMPTY if name != 'dense' else 1, S.BIG_OFFSET)):
            x = case.expected(tail=tail, row_offset=row_offset)
            (n_meth, n_total, first), extras, index = host_reduction(case, tail, row_offset)
            assert index.n == x.n_sites == len(n_meth), name
            assert np.array_equal(n_meth, x.n_meth) and np.array_equal(n_total, x.n_total) and np.array_equal(first, x.first), name
            assert np.flatnonzero(extras['records']).tolist() == x.cross and extras['rows'] == x.extras, name
            assert (x.first[x.n_total == 0] == S.INT64_MAX).all() and (x.first[x.n_total > 0] < S.INT64_MAX).all()
            for key, number in x.number.items():
                assert index.locate(number) == key


def test_bed_from_the_restated_counts_equals_make_bed_on_the_diffs_text(cases, tmp_path, monkeypatch):
    """The multi-contig case with cross-contig records (its rows are extras of write_bed_from_counts): records -> .diffs rows
    (Finisher) -> make_bed.main against restated counts -> write_bed_from_counts, equal bytes."""
    from mcaller_amd import extract_contexts as ec
    from tests import helpers as H
    case = cases['motif']
    rec, prob, nan = case.records()
    assert not nan[(rec.info[:rec.n] & _lib.I_TOO_MANY) == 0].any()          # every call is a row the formatter prints
    x = case.expected()
    assert len(x.extras) >= 2 and len(set(c for c, _, _ in x.counted)) >= 5

    class P(object):
        pass
    P.table, P.ref, P.qual = case.table, case.ref, case.qual
    P.qual_obj = [np.float64(q) for q in case.qual]
    P.fatal = None
    fin = ec.Finisher(P, case.k, 'A', False, modelset=H.load_modelset('r95'), tail_chrom=case.ref.names[case.tail])
    with contextlib.redirect_stdout(io.StringIO()):
        assert fin.run(rec) is None
    diffs = tmp_path / 'sites.eventalign.diffs.6'
    diffs.write_bytes(fin.text())
    index = make_bed.SiteIndex(case.ref.meth, case.n_contigs)
    monkeypatch.chdir(tmp_path)
    for depth, thresh in ((1, 0.0), (2, 0.5)):
        with contextlib.redirect_stdout(io.StringIO()):
            make_bed.main(['-f', diffs.name, '-d', str(depth), '-t', str(thresh)])
        want = (tmp_path / 'sites.methylation.summary.bed').read_text()
        out = tmp_path / 'restated.bed'
        make_bed.write_bed_from_counts(str(out), x.n_meth, x.n_total, x.first, index, case.ref.names, case.ref.meth, case.k, depth, thresh,
                                       extras=x.extras)
        assert out.read_text() == want and want.count('\n') >= 3
        # (the rows of the cross-contig records are there: chrom is the contig of the closing row)
        assert depth > 1 or all(any(line.split('\t')[:2] == [e[0], str(e[1])] for line in want.splitlines()) for e in x.extras)
