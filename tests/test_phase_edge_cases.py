"""tests/phase_edge_cases.py held to its claims, on the CPU: every builder reaches the edge it names (read lengths and arrival, head
lines, count fields, tables at the option edges, duplicate counts, windows); on every case the GPU tests expect the device to make,
the host statement's bytes equal the brute force's and `servable` is []; every value decline gets from mc_fisher.h's host build the
status bit it is built for; every line decline gets from the host statement the error or the output the GPU test expects behind it.
A case that fails `servable` is not skipped on the GPU: its seed is changed here."""
import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import phase_reads as P
from tests import phase_cases as K
from tests import phase_edge_cases as E
from tests.test_phase_cases import read_lengths, window


@pytest.fixture(scope='module')
def made(tmp_path_factory):
    """name -> (path, text, options, claims, brute_tables' result): every served case is built and counted once."""
    out = {}
    for name, make in E.SERVED.items():
        text, opt, claims = make()
        p = K.write(tmp_path_factory.mktemp('case'), text)
        out[name] = (p, text, opt, claims, K.brute_tables(p, opt['depth'], opt['max_dist']))
    return out


def tables_by_pos(tables):
    return {(int(a[1]), int(b[1])): tuple(t) for (a, b), t in tables.items()}


@pytest.mark.parametrize('name', sorted(E.SERVED))
def test_host_equals_brute_and_the_device_has_no_reason_to_decline(made, name):
    p, text, opt, claims, (kept, _, _, _, _) = made[name]
    fdr = name in E.FDR
    for threshold in (0.3, 0.0, float('inf')) if len(text) < 100000 else (0.3,):
        want = K.brute(p, fdr=fdr, threshold=threshold, **opt)
        got = P._rows(p, fdr=fdr, threshold=threshold, want_reads=True, want_bed=True, **opt)
        assert got == want[:4], (name, threshold)
    if 'window' in claims:
        assert window(E.unfilled(kept), opt['max_dist']) == claims['window'], name
    if 'sites' in claims:
        assert len(kept) == claims['sites'], name
    assert E.servable(p, opt, fdr=fdr, brute=want) == [], name


def test_long_reads_arrive_in_no_order(made):
    assert E.LONG == (65, 128, 129, 1000, 1025, 2047, 2048) and (E.WAVE, E.GROUP) == (_lib.PHASE_WAVE_ROWS, _lib.PHASE_GROUP_ROWS)
    outputs = []
    for name in ('long_shuffled', 'long_reversed'):
        p, text, opt, claims, (kept, sites, tables, _, duplicates) = made[name]
        lines = text.decode().splitlines()
        n = read_lengths(text)
        assert len(lines) == claims['lines'] == 6762 and duplicates == 0
        assert [n[('chr1', 'len%d' % k, '+')] for k in E.LONG] == list(E.LONG) and sorted(n.values())[:8] == [40] * 8 and len(n) == 15
        # the 2048th position has one read: the longest read's last row stands at a site that is not kept
        assert len(kept) == claims['sites'] == 2047 and sites[('chr1', '3047', '+')][1] == 1 and ('chr1', '3047', '+') not in kept
        assert sum(sum(t) for t in tables.values()) == claims['instances'] == 20193
        for k in E.LONG:
            at = [(no, int(l.split('\t')[2])) for no, l in enumerate(lines) if l.split('\t')[1] == 'len%d' % k]
            positions = [pos for _, pos in at]
            assert positions != sorted(positions) and sorted(positions) == list(range(1000, 1000 + k)), (name, k)
            # the rows lie in at least three 256-line staging tiles; a reversed read is one run of lines, which fewer than 513 rows
            # cannot spread that far: there every row arrives in front of the row before it in the genome, and that is all
            tiles = {no // 256 for no, _ in at}
            assert len(tiles) >= (3 if name == 'long_shuffled' or k > 512 else 1), (name, k, tiles)
            if name == 'long_reversed':
                assert positions == sorted(positions, reverse=True)
        if name == 'long_shuffled':                                     # ... and in no order at all: ascents and descents
            steps = np.sign(np.diff([int(l.split('\t')[2]) for l in lines if l.split('\t')[1] == 'len2048']))
            assert min((steps > 0).sum(), (steps < 0).sum()) > 900
        rows, reads, bed, fig = P._rows(p, want_reads=True, want_bed=True, threshold=0.3, **opt)
        assert fig['n_pairs'] == rows.count(b'\n') > 2000 and fig['n_reads'] == 15
        outputs.append(tuple(sorted(o.splitlines()) for o in (rows, reads, bed)))
    # the same lines in both arrivals, each in the order of its own file's first rows
    assert outputs[0] == outputs[1]
    assert sorted(made['long_shuffled'][1].splitlines()) == sorted(made['long_reversed'][1].splitlines())


def test_duplicates(tmp_path):
    for variant in ('one', 'two', 'unkept', 'by_duplicate', 'no_site'):
        text, opt, claims = E.case_duplicate(variant)
        p = K.write(tmp_path, text)
        lines = text.decode().splitlines()
        kept, sites, _, calls, duplicates = K.brute_tables(p, opt['depth'], opt['max_dist'])
        fig = P._rows(p, **opt)[3]
        assert duplicates == fig['n_duplicates'] == claims['duplicates'], variant
        # every duplicate row: the read key, pos, and the first row of the combination, which says the opposite
        seen, later = {}, []
        for no, l in enumerate(lines):
            f = l.split('\t')
            key = (f[0], f[1], f[5], f[2])
            if key in seen:
                later.append(no)
                assert (lines[seen[key]].split('\t')[6] == 'm6A') != (f[6] == 'm6A')
            seen.setdefault(key, no)
        assert len(later) == claims['duplicates'] and (claims['line'] is None or min(later) == claims['line']), (variant, later)
        if variant in ('one', 'two'):
            assert {lines[no].split('\t')[1] for no in later} == {'len1025'} and read_lengths(text)[('chr1', 'len1025', '+')] == claims['read_rows']
            assert later == [4000, 5500][:claims['duplicates']]
        if variant == 'unkept':
            assert sites[('chr1', '710', '-')][1] == 5 and sum(1 for l in lines if l.split('\t')[2] == '710') == 6 < opt['depth'] and len(kept) == 2
        if variant == 'by_duplicate':
            assert sites[('chr1', '710', '-')][1] == opt['depth'] - 1 and sum(1 for l in lines if l.split('\t')[2] == '710') == opt['depth']
            assert len(kept) == fig['n_sites'] == claims['host_sites'] == 2 and claims['device_sites'] == 3
        if variant == 'no_site':
            assert kept == [] and fig['n_sites'] == 0 and P._rows(p, want_reads=True, want_bed=True, **opt)[:3] == (b'', b'', b'')
            assert E.servable(p, opt) == []
        else:
            assert [r[0] for r in E.servable(p, opt)] == ['duplicate'], variant


def test_count_fields_at_capacity(made):
    top = [0, 0, 0, 0]
    for name in E.DEEP:
        p, text, opt, claims, (kept, sites, tables, _, duplicates) = made[name]
        assert len(kept) == claims['sites'] and all(sites[s][1] == K.MAX_DEPTH == 65535 for s in kept) and duplicates == 0
        got = tables_by_pos(tables)
        assert [got[ab] for ab in sorted(got)] == claims['tables'] and all(sum(t) == 65535 for t in got.values())
        written = K.brute(p, fdr=True, **opt)[4]
        assert sorted(tuple(t) for t, _ in written) == sorted(claims['tables'])             # every one of them is written
        for t in claims['tables']:
            top = [max(a, b) for a, b in zip(top, t)]
    assert (2, 1, 1, 65531) in E.DEEP_TABLES['deep'] and (1, 2, 65530, 2) in E.DEEP_TABLES['deep']
    assert (65531, 1, 1, 2) in E.DEEP_TABLES['deep_flipped'] and (2, 65530, 2, 1) in E.DEEP_TABLES['deep_flipped']
    assert min(top) >= 65530 and E.DEEP_TABLES['deep_balanced'] == [(16384, 16384, 16384, 16383)]
    assert len(made['deep'][1].splitlines()) == 196605 and 8.5e6 < len(made['deep'][1]) < 8.7e6


def test_keys_equal_in_all_but_one_field(made):
    p, text, opt, claims, (kept, _, tables, calls, duplicates) = made['near_keys']
    groups = {(s[0], s[2]) for s in kept}
    assert groups == {(c, s) for c, s, _ in E.NEAR_GROUPS} and len(groups) == claims['groups'] == 7 and duplicates == 0
    assert len(kept) == claims['sites'] == 42 and len({s[1] for s in kept}) == 6 and len(calls) == claims['reads'] == 84
    reads = set(calls)
    assert {('chrA', 'n3', '+'), ('chrA', 'n3', '-'), ('chrB', 'n3', '+')} <= reads                  # strand alone, chrom alone
    assert {('c', '1r3', '+'), ('c1', 'r3', '+')} <= reads                                            # the boundary of chrom and read
    assert {('chr1', 'm3', '+'), ('chr', 'm3', '1+')} <= reads                                        # the boundary of chrom and strand
    assert len({c + r + s for c, r, s in reads}) < len(reads) and len({c + s for c, s in groups}) < len(groups)
    assert all(len(mine) == 6 for mine in calls.values())
    # every pair of every group is written, and no two groups have the same tables
    written = K.brute(p, **opt)[4]
    assert len(tables) == len(written) == claims['rows'] == 63
    per_group = {}
    for (a, b), t in tables.items():
        per_group.setdefault((a[0], a[2]), {})[(a[1], b[1])] = tuple(t)
    assert len(per_group) == 7 and len({tuple(sorted(g.items())) for g in per_group.values()}) == 7
    # the labels of two reads with one name differ somewhere: a merge of the keys would change a table, not only make duplicates
    assert calls[('chrA', 'n3', '+')] != calls[('chrA', 'n3', '-')] and calls[('chrA', 'n3', '+')] != calls[('chrB', 'n3', '+')]


def test_group_head_lines(made):
    for form, name in (('full', 'group_lines_full'), ('257', 'group_lines_257'), ('65537', 'group_lines_65537')):
        p, text, opt, claims, (kept, sites, tables, _, duplicates) = made[name]
        lines = text.decode().splitlines()
        assert len(lines) == claims['lines'] == {'full': 65856, '257': 257, '65537': 65537}[form] and duplicates == 0
        is_kept = set(kept)
        heads = {}
        for no, l in enumerate(lines):
            f = l.split('\t')
            if (f[0], f[2], f[5]) in is_kept:
                heads.setdefault(f[0], no)
        assert {c: heads[c] for c in claims['heads']} == claims['heads'], (form, heads)
        assert len({h % 256 for h in claims['heads'].values()}) == 1
        if form == 'full':
            assert claims['heads'] == {'chrA': 0, 'chrB': 256, 'chrC': 65536} and 'chrF' not in heads and len(kept) == 60
            assert len({h % 65536 for h in (0, 65536)}) == 1 and opt['depth'] > 1
            assert all(sorted(int(s[1]) for s in kept if s[0] == c) == [100 + 3 * i for i in range(20)] for c in ('chrA', 'chrB', 'chrC'))
            assert len(K.brute(p, **opt)[4]) > 60
        else:
            # the last group's only kept site is the last line, at a position inside chrA's: a key without its upper bits sorts among chrA's
            last = 'chrB' if form == '257' else 'chrC'
            assert opt['depth'] == 1 and heads[last] == len(lines) - 1 and sum(1 for s in kept if s[0] == last) == 1
            pos = [int(s[1]) for s in kept if s[0] == last][0]
            mine = sorted(int(s[1]) for s in kept if s[0] == 'chrA')
            assert mine[0] < pos <= mine[-1] and mine[-1] - mine[0] <= opt['max_dist'] and claims['window'] == len(mine) - 1 == 15
            assert len(K.brute(p, **opt)[4]) > 30
            fill = [int(s[1]) for s in kept if s[0] == 'chrF']                     # no filler site has a site within max_dist: E.unfilled
            assert len(fill) == len(set(fill)) == (65024 if form == '65537' else 0) and all(q % 10000 == 0 for q in fill) and opt['max_dist'] < 10000
    # the skip rule of ph_sort_sites at these line counts: the pass of bits 40 .. 47 runs from 257 lines on, of 48 .. 55 from 65537
    ran = lambda n_lines: [sh for sh in range(32, 64, 8) if (n_lines >> (sh - 32)) != 0]
    assert ran(257) == [32, 40] and ran(65537) == [32, 40, 48] and ran(65856) == [32, 40, 48]


def test_option_and_position_edges(made):
    for name in ('max_dist_2^31-1', 'max_dist_2^31', 'max_dist_10^12'):
        p, text, opt, claims, (kept, _, tables, _, _) = made[name]
        assert len(kept) == 40 and len({(s[0], s[2]) for s in kept}) == 1 and len(tables) == 40 * 39 // 2 and claims['window'] == 39
        assert text == made['max_dist_2^31'][1] and len(K.brute(p, **opt)[4]) > 100
    assert [made[n][2]['max_dist'] for n in ('max_dist_2^31-1', 'max_dist_2^31', 'max_dist_10^12')] == [2 ** 31 - 1, 2 ** 31, 10 ** 12]
    p, _, opt, claims, (kept, _, tables, _, _) = made['far_positions']
    assert [s[1] for s in sorted(kept, key=lambda s: int(s[1]))] == claims['positions'] == ['0', '999999999'] and opt['max_dist'] == 10 ** 12
    rows, _, bed, fig = P._rows(p, want_reads=True, want_bed=True, threshold=0.0, **opt)
    assert fig['n_pairs'] == 1 and rows.split(b'\t')[2:4] == [b'0', b'999999999'] and fig['n_linked'] == 2
    assert sorted(l.split(b'\t')[1:3] for l in bed.splitlines()) == [[b'0', b'1'], [b'999999999', b'1000000000']]
    # tables exactly at --min_reads and --min_margin, and one below each
    for name, margin, want in (('table_edges_margin_2', 2, [1000, 3000]), ('table_edges_margin_1', 1, [1000, 3000, 4000])):
        p, _, opt, claims, (kept, _, tables, _, _) = made[name]
        got = tables_by_pos(tables)
        assert {a: got[(a, a + 5)] for a in E.EDGE_TABLES} == E.EDGE_TABLES and len(got) == 5 and opt['min_margin'] == margin
        assert sum(E.EDGE_TABLES[1000]) == opt['min_reads'] == sum(E.EDGE_TABLES[2000]) + 1
        assert [min(t[0] + t[1], t[2] + t[3], t[0] + t[2], t[1] + t[3]) for t in E.EDGE_TABLES.values()] == [5, 4, 2, 1, 0]
        rows = P._rows(p, **opt)[0].decode().splitlines()
        assert sorted(int(r.split('\t')[2]) for r in rows) == want == claims['written']
    p, _, opt, claims, (kept, _, tables, _, _) = made['no_pair']
    rows, reads, bed, fig = P._rows(p, fdr=True, want_reads=True, want_bed=True, threshold=0.0, **opt)
    assert opt['min_reads'] == 2 ** 40 and len(kept) == claims['sites'] and tables
    assert (rows, bed) == (b'', b'') and reads.count(b'\n') == fig['n_reads'] == claims['reads'] and fig['n_pairs'] == fig['n_linked'] == 0
    # --threshold 0.0 links every site of a written pair, inf none
    p, _, opt, _, _ = made['near_keys']
    rows, _, bed, fig = P._rows(p, want_bed=True, threshold=0.0, **opt)
    in_rows = {(f[0], f[1], pos) for f in (r.split('\t') for r in rows.decode().splitlines()) for pos in f[2:4]}
    assert {(f[0], f[5], f[1]) for f in (l.split('\t') for l in bed.decode().splitlines())} == in_rows and fig['n_linked'] == len(in_rows) == 42
    assert P._rows(p, want_bed=True, threshold=float('inf'), **opt)[2] == b''


def test_value_declines_have_the_status_they_are_built_for(tmp_path):
    assert (E.FE_FAR_TAIL, E.FE_SELECT) == (2, 4)
    for table, want in ((E.SERVED_TABLE, 0), (E.FAR_TABLE, E.FE_FAR_TAIL), (E.DEEPER_TABLE, E.FE_FAR_TAIL)):
        n11, n10, n01, n00 = table
        st, l, bound = _lib.fisher_exact(n11, n11 + n10, n01, n01 + n00)
        assert st == want, (table, st, l)
        assert (l < -250.0) == (want != 0)
    text, opt, claims = E.case_far_tail('served')
    p = K.write(tmp_path, text)
    rows = P._rows(p, **opt)[0].decode().splitlines()
    assert len(rows) == 1 and rows[0].split('\t')[4:] == ['842', '420', '1', '1', '420', '0.995', claims['printed']] and claims['printed'] == '246.357'
    for which, far_pos in (('one', 3000), ('two', 5000), ('deeper', 3000)):
        text, opt, claims = E.case_far_tail(which)
        p = K.write(tmp_path, text)
        tables = tables_by_pos(K.brute_tables(p, opt['depth'], opt['max_dist'])[2])
        far = {a: t for (a, _), t in tables.items() if t != E.SERVED_TABLE}
        assert tables[(1000, 1005)] == E.SERVED_TABLE and set(far.values()) == {E.DEEPER_TABLE if which == 'deeper' else E.FAR_TABLE}
        assert len(far) == (2 if which == 'two' else 1)
        # the first row of site A of the far pair that stands first in the file -- which is not the first in the genome
        heads = {a: E.head_line(text, 'chr1', a) for a in far}
        assert claims['line'] == min(heads.values()) == heads[far_pos] == 2 * 842 and E.head_line(text, 'chr1', far_pos + 5) > claims['line']
        assert [r[0] for r in E.servable(p, opt)] == ['far_tail'] * len(far)
        assert P._rows(p, **opt)[3]['n_pairs'] == 1 + len(far)                      # the host statement writes them all


def test_line_declines_on_the_host(tmp_path):
    cases = E.line_declines()
    assert len(cases) == 12
    base, opt, _ = K.case_shuffled()
    p0 = K.write(tmp_path, base, 'base.diffs')
    for name, (text, opt, reason, line, error) in cases.items():
        p = K.write(tmp_path, text)
        assert reason in _lib.CMP_DECLINE and 0 <= line < len(text.split(b'\n')), name
        if error is not None:
            with pytest.raises(ValueError) as e:
                P._rows(p, **opt)
            assert error in str(e.value) and ('line %d:' % (line + 1)) in str(e.value), (name, str(e.value))
        else:
            fig = P._rows(p, **opt)[3]
            assert fig['n_duplicates'] == 0 and fig['n_sites'] >= 29, name
    raw = {name: c[0].split(b'\n') for name, c in cases.items()}
    assert any(b >= 0x80 for b in raw['high_byte'][137]) and raw['carriage_return'][137].endswith(b'\r') and len(raw['long_line'][420]) > 65535
    assert raw['six_fields'][137].count(b'\t') == 5 and raw['nine_fields'][137].count(b'\t') == 8
    orig = base.split(b'\n')[137].split(b'\t')[2]
    assert [raw[n][137].split(b'\t')[2] for n in ('pos_leading_zeros', 'pos_sign', 'pos_ten_digits', 'pos_empty')] == [b'00' + orig, b'+' + orig, b'1234567890', b'']
    # a carriage return in front of the newline is no byte of the host's line: the host's output is that of the text without it
    assert P._rows(K.write(tmp_path, cases['carriage_return'][0]), **opt)[0] == P._rows(p0, **opt)[0]
