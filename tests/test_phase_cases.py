"""Every builder of tests/phase_cases.py held to what it claims -- depths, read lengths, distances and windows exactly at their
edges -- and every case the GPU tests expect the device to make shown, on the HOST builds of mc_fisher.h and mc_bh.h
(_lib.fisher_exact, _lib.bh_adjust), to carry no Fisher status bit, no MC_BH_TIE and no nlp within its bound of a rounding tie: a
case that fails this is not skipped on the GPU, its seed is changed here."""
import numpy as np
import pytest

from mcaller_amd import _lib
from tests import phase_cases as K

ALL_CASES = dict(K.DEVICE_CASES, counter_memory=K.case_counter_memory, many_reads=K.case_many_reads,
                 depth_cap=lambda: K.case_depth_cap(400), duplicate_base=K.case_shuffled)


@pytest.fixture(scope='module')
def made(tmp_path_factory):
    """name -> (path, text, options, claims, brute_tables' result): every case is built and counted once."""
    out = {}
    for name, make in ALL_CASES.items():
        text, opt, claims = make()
        p = K.write(tmp_path_factory.mktemp(name), text)
        out[name] = (p, text, opt, claims, K.brute_tables(p, opt['depth'], opt['max_dist']))
    return out


def window(kept, max_dist):
    """W as the device reports it: the most kept sites of a site's chrom and strand behind it within max_dist, at least 1."""
    best = 1
    for a in kept:
        best = max(best, sum(1 for b in kept if (a[0], a[2]) == (b[0], b[2]) and 0 < int(b[1]) - int(a[1]) <= max_dist))
    return best


def read_lengths(text):
    n = {}
    for line in text.decode().splitlines():
        f = line.split('\t')
        n[(f[0], f[1], f[5])] = n.get((f[0], f[1], f[5]), 0) + 1
    return n


def test_windows_are_what_the_cases_claim(made):
    for name, (_, _, opt, claims, (kept, _, _, _, duplicates)) in made.items():
        assert duplicates == 0, name
        if 'window' in claims:
            assert window(kept, opt['max_dist']) == claims['window'], name


def test_read_lengths_stand_on_the_kernels_edges(made):
    _, text, _, claims, (kept, _, _, _, _) = made['read_lengths']
    n = read_lengths(text)
    assert claims['lengths'] == (1, 2, K.WAVE - 1, K.WAVE, K.WAVE + 1, K.GROUP) and (K.WAVE, K.GROUP) == (_lib.PHASE_WAVE_ROWS, _lib.PHASE_GROUP_ROWS)
    assert [n[('chr1', 'len%d' % k, '+')] for k in claims['lengths']] == list(claims['lengths'])
    assert max(n.values()) == K.GROUP and len(kept) == K.GROUP and sorted(v for v in n.values() if v == 40) == [40] * 8
    beyond = read_lengths(K.case_read_lengths(lengths=(5, K.GROUP + 1))[0])
    assert max(beyond.values()) == K.GROUP + 1


def test_the_shuffled_reads_span_both_tiles(made):
    for name in ('shuffled', 'shuffled_no_newline'):
        _, text, _, claims, _ = made[name]
        lines = text.decode().splitlines()
        assert len(lines) == claims['lines'] == 420 and text.endswith(b'\n') == (name == 'shuffled')
        where = {}
        for no, line in enumerate(lines):
            where.setdefault(line.split('\t')[1], set()).add(no // 256)
        assert len(where) == 14 and all(tiles == {0, 1} for tiles in where.values())
        positions = [int(l.split('\t')[2]) for l in lines]
        assert positions != sorted(positions)


def test_distances_at_the_edge(made):
    _, _, opt, claims, (kept, _, tables, _, _) = made['distance_edge']
    a, b, c = (('chr1', str(p), '+') for p in claims['positions'])
    assert kept and set(kept) == {a, b, c}
    assert int(b[1]) - int(a[1]) == opt['max_dist'] and int(c[1]) - int(b[1]) == opt['max_dist'] + 1
    assert set(tables) == {(a, b)} and sum(tables[(a, b)]) == 24


def test_groups_do_not_pair_across(made):
    _, _, _, claims, (kept, _, tables, _, _) = made['strands_and_chroms']
    assert len({(s[0], s[2]) for s in kept}) == claims['groups'] == 4 and len({s[1] for s in kept}) == 6 and len(kept) == 24
    assert tables and all((a[0], a[2]) == (b[0], b[2]) for a, b in tables)


def test_the_site_below_the_depth(made):
    _, _, opt, claims, (kept, sites, tables, _, _) = made['below_depth_between']
    assert sorted(int(s[1]) for s in kept) == claims['kept'] and sites[('chr1', '710', '-')][1] == 5 < opt['depth'] <= 18 == sites[('chr1', '700', '-')][1]
    assert list(tables) == [(('chr1', '700', '-'), ('chr1', '720', '-'))]


def test_depths_at_the_cap():
    for n in (K.MAX_DEPTH, K.MAX_DEPTH + 1):
        text, opt, claims = K.case_depth_cap(n)
        lines = text.split(b'\n')
        assert claims['depth'] == n and sum(1 for l in lines if b'\t500\t' in l) == n and sum(1 for l in lines if b'\t501\t' in l) == 24
        assert lines[0].split(b'\t')[2] == b'500'                        # the deep site's first row is line 0
    assert K.MAX_DEPTH == _lib.PHASE_MAX_DEPTH == 65535


def test_the_budget_cases(made):
    _, text, opt, claims, (kept, _, _, _, _) = made['counter_memory']
    assert len(kept) == 300 and len(text) < 300000 and 300 * claims['window'] * 65 > (1 << 20)
    _, text, _, claims, (kept, _, _, calls, _) = made['many_reads']
    assert len(kept) == 4 and len(calls) == claims['reads'] == 120 > 64


def nlp_tie(L, bound):
    """mc_tstat.h's ts_tie_between on the printed -log10 p, as kr_finish runs it."""
    lo, hi = max(-L - bound, 0.0), max(-L + bound, 0.0)
    lo, hi = np.rint(lo * 1000.0), np.rint(hi * 1000.0)
    return lo != hi or np.signbit(lo) != np.signbit(hi)


@pytest.mark.parametrize('name', sorted(ALL_CASES))
def test_no_status_bit_and_no_tie_on_the_host_builds(made, name):
    p, _, opt, _, _ = made[name]
    written = K.brute(p, **opt)[4]
    if name in K.DEVICE_CASES:
        assert written, name
    if not written:
        return
    t = np.asarray([table for table, _ in written], dtype=np.int64)
    L, bound, status = _lib.fisher_exact(t[:, 0], t[:, 0] + t[:, 1], t[:, 2], t[:, 2] + t[:, 3])
    assert not status.any(), (name, status)
    assert not any(nlp_tie(l, b) for l, b in zip(L, bound)), name
    assert np.max(np.abs(L - np.asarray([l for _, l in written]))) <= np.max(bound)
    _, _, bh_status = _lib.bh_adjust(L, bound)
    assert bh_status == 0, (name, bh_status)
