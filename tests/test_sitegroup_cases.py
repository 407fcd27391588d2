"""tests/sitegroup_cases.py held to its claims, on the CPU: on every case the host statement's bytes equal the brute force's
(currents_cases.brute_rows against compare_currents._rows, cluster_cases.brute_rows against cluster_sites._rows); the case reaches
the edge it names; `servable` is [] wherever tests/test_gpu_sitegroup_edges.py demands the device's own bytes; and every decline case
gets from the host builds the status bits it is built for."""
import numpy as np

from mcaller_amd import _lib
from mcaller_amd import cluster_sites as CS
from mcaller_amd import compare_currents as CC
from tests import cluster_cases as KS
from tests import currents_cases as K
from tests import sitegroup_cases as G


def host_equals_brute(tmp_path, native, control, depth, fdr=False, by=None, threshold=2.0):
    """-> (rows, bed, n) of the host statement, equal to the brute force's."""
    p1, p2 = K.files(tmp_path, native, control)
    rows, bed, n, n_sig = CC._rows(p1, p2, depth, fdr, by or 'mwu', threshold, by is not None)
    want_rows, want_bed, _ = K.brute_rows(native, control, depth, fdr, by, threshold)
    assert rows == want_rows and (bed or b'') == want_bed and n == rows.count(b'\n') and n_sig == want_bed.count(b'\n')
    return rows, bed or b'', n


def cluster_equals_brute(tmp_path, text, depth=2, **kw):
    p = KS.write(tmp_path, text)
    rows, bed, n, n_mixed = CS._rows(p, depth, 256, 'correlation', kw.get('mixed', False), kw.get('min_minor', 0.2), kw.get('min_gap', 2.0))
    want_rows, want_bed = KS.brute_rows(text, depth=depth, **kw)
    assert rows == want_rows and (bed or b'') == want_bed and n == rows.count(b'\n')
    return rows, bed or b'', n


def test_unbalanced(tmp_path):
    native, control = G.unbalanced()
    sites = K.brute_sites(native, control, 2)
    assert [(len(x), len(y)) for _, _, x, y in sites] == G.UNBALANCED and all(x.shape[1] == 1 for _, _, x, _ in sites)
    assert [len(x) + len(y) for _, _, x, y in sites] == [64, 64, 65, 65, 512, 513, 8192, 8192] and max(G.UNBALANCED[-1]) + 2 == G.TW_MAX_N
    rows, _, n = host_equals_brute(tmp_path, native, control, 2, fdr=True)
    assert n == 8 and all(len(r.split('\t')) == 7 + 1 + 8 for r in rows.decode().splitlines())
    assert G.servable(native, control, 2, fdr=True) == []


def test_wide(tmp_path):
    native, control = G.wide()
    sites = K.brute_sites(native, control, 3)
    assert len(sites) == 12 and all(x.shape[1] == G.WIDE_C == 24 for _, _, x, _ in sites)
    rows, _, n = host_equals_brute(tmp_path, native, control, 3, fdr=True)
    assert all(3 <= len(v) <= 8 for _, _, x, y in sites for v in (x, y)) and len(set((len(x), len(y)) for _, _, x, y in sites)) > 4
    printed = sorted(float(r.split('\t')[-1]) for r in rows.decode().splitlines())      # nlq_ks: some rows reach the largest, others do not
    _, bed, _ = host_equals_brute(tmp_path, native, control, 3, fdr=True, by='ks', threshold=printed[-1])
    assert n == 12 and 0 < bed.count(b'\n') < 12 and printed[0] < printed[-1]
    assert len(max(rows.splitlines(), key=len)) > 200                 # a row far longer than any of the pipelines' own tests
    assert G.servable(native, control, 3, fdr=True) == []


def test_keys(tmp_path):
    native, control = G.keys_pair()
    rows, _, n = host_equals_brute(tmp_path, native, control, 3)
    nat_ctx, nat_order = G.first_contexts(native)
    con_ctx, _ = G.first_contexts(control)
    assert n == 9 and set(nat_ctx) == set(G.KEYS) | {G.KEY_NATIVE_ONLY} and set(con_ctx) == set(G.KEYS) | {G.KEY_CONTROL_ONLY}
    # two pairs of keys whose chrom and pos bytes are equal when they stand behind one another
    glued = [(a, b) for a in G.KEYS for b in G.KEYS if a < b and a[0] != b[0] and a[0] + str(a[1]) + a[2] == b[0] + str(b[1]) + b[2]]
    assert sorted(glued) == [(('chr', 1100, '+'), ('chr1', 100, '+')), (('chr1', 10, '+'), ('chr11', 0, '+'))]
    assert ('chr1', 100, '-') in G.KEYS                               # and a pair that differs in the strand alone
    # a context per row, in both files; the lines of the sites are interleaved; head rows of 7 and of 8 fields
    for one in (native, control):
        lines = [l.split('\t') for l in one.decode().splitlines()]
        assert len(set(f[3] for f in lines)) == len(lines) and all(len(f[3]) == 11 for f in lines)
        keys = [(f[0], f[2], f[5]) for f in lines]
        assert sum(a != b for a, b in zip(keys, keys[1:])) > len(set(keys))
    heads = {}
    for l in native.decode().splitlines():
        f = l.split('\t')
        heads.setdefault((f[0], int(f[2]), f[5]), len(f))
    assert sorted(heads[k] for k in G.KEYS).count(7) == 4 and sorted(heads[k] for k in G.KEYS).count(8) == 5
    got = [r.split('\t') for r in rows.decode().splitlines()]
    assert [(r[0], int(r[1]), r[4]) for r in got] == [k for k in nat_order if k in G.KEYS]
    assert all(r[3] == nat_ctx[(r[0], int(r[1]), r[4])] for r in got)
    ends = {(r[0], r[1]): r[2] for r in got}
    assert ends[('c', '0')] == '1' and ends[('c', '999999999')] == '1000000000' and ends[('chr11', '0')] == '1'
    assert G.servable(native, control, 3) == []
    # the one-file version: the native file's ten keys, each a site of cluster_sites
    text = G.keys_text()
    rows, _, n = cluster_equals_brute(tmp_path, text, depth=2)
    ctx, order = G.first_contexts(text)
    got = [r.split('\t') for r in rows.decode().splitlines()]
    assert n == 10 and [(r[0], int(r[1]), r[4]) for r in got] == order and all(r[3] == ctx[(r[0], int(r[1]), r[4])] for r in got)


def test_many(tmp_path):
    native, control = G.many_pair()
    rows, _, n = host_equals_brute(tmp_path, native, control, 2, by='t', threshold=0.0)
    assert 1100 <= n < 1500 and n > 1024
    nat_ctx, nat_order = G.first_contexts(native)
    con_ctx, _ = G.first_contexts(control)
    assert len(nat_ctx) == 1500 and len(set(con_ctx) - set(nat_ctx)) > 100 and len(set(nat_ctx) - set(con_ctx)) > 100
    assert sorted(nat_order) != nat_order                             # shuffled as a whole: the keys' first rows come in no order
    # with --fdr every printed q is at least 0.0: every row is in the bed (the brute force's O(m^2) q-values are left to `wide`)
    p1, p2 = K.files(tmp_path, native, control)
    rows_fdr, bed, n_fdr, n_sig = CC._rows(p1, p2, 2, True, 't', 0.0, True)
    assert n_fdr == n_sig == n and [r.split(b'\t')[:7 + 1 + 4] for r in rows_fdr.splitlines()] == [r.split(b'\t') for r in rows.splitlines()]
    assert G.servable(native, control, 2, fdr=True) == []
    text = G.many_text()
    _, bed, n = cluster_equals_brute(tmp_path, text, depth=2, mixed=True, min_minor=0.0, min_gap=0.0)
    assert 1024 < n < 1500 and bed.count(b'\n') == n


def rows_of(one_text, key):
    """the 0-based lines of a text that carry the key"""
    return [i for i, l in enumerate(one_text.decode().splitlines()) if (l.split('\t')[0], int(l.split('\t')[2]), l.split('\t')[5]) == key]


def test_deep_unkept_and_kept(tmp_path):
    native, control, line = G.deep_pair(kept=False)
    _, _, n = host_equals_brute(tmp_path, native, control, 2)
    assert n == 3 and [len(x) + len(y) for _, _, x, y in K.brute_sites(native, control, 2)] == [6, 6, 6]
    alone = ('chrE', 90, '-')
    assert len(rows_of(native, G.DEEP_KEY)) == G.DEEP_NATIVE > G.TW_MAX_N and rows_of(native, G.DEEP_KEY)[0] == line == 3
    assert len(rows_of(control, G.DEEP_KEY)) == 1
    assert len(rows_of(control, alone)) == G.DEEP_CONTROL_ALONE > G.TW_MAX_N and not rows_of(native, alone)
    assert G.servable(native, control, 2) == []
    # the twin: the same text with one more control row for the deep key, which makes it a site, and one over the cap
    native2, control2, line2 = G.deep_pair(kept=True)
    at = rows_of(control2, G.DEEP_KEY)
    twin_lines = control2.decode().splitlines(True)
    assert native2 == native and line2 == line and len(at) == 2 and ''.join(twin_lines[:at[1]] + twin_lines[at[1] + 1:]).encode() == control
    rows2, _, n2 = host_equals_brute(tmp_path, native2, control2, 2)
    assert n2 == 4 and rows2.decode().splitlines()[1].split('\t')[:7] == ['chrE', '50', '51', 'GATCMGATCGA', '+', '8200', '2']
    assert G.servable(native2, control2, 2) == [(('chrE', '50', '+'), 'depth')]


def test_spellings(tmp_path):
    for token, value in G.SPELLED:
        assert float(token) == value and _lib.parse_double(token) == value, token
        assert np.copysign(1.0, float(token)) == np.copysign(1.0, value)
    assert sum(repr(float(t)) != t for t, _ in G.SPELLED) >= 13
    for form in ('+1.5', '.5', '5.', '1e-3', '1E2', '-0.0'):
        assert form in [t for t, _ in G.SPELLED]
    assert any(len(t.lstrip('+-0.').split('e')[0].replace('.', '')) == 19 for t, _ in G.SPELLED)
    native, control, native_twin, control_twin = G.spellings_pair()
    assert native != native_twin and control != control_twin
    used = set()
    for spelled, twin in ((native, native_twin), (control, control_twin)):
        for a, b in zip(spelled.decode().splitlines(), twin.decode().splitlines()):
            fa, fb = a.split('\t'), b.split('\t')
            ta, tb = fa[4].split(','), fb[4].split(',')
            assert fa[:4] + fa[5:] == fb[:4] + fb[5:] and len(ta) == len(tb) == G.SPELLINGS_C + 1
            assert all(float(x) == float(y) and repr(float(x)) == y for x, y in zip(ta, tb))
            assert len(set(len(t) for t in ta)) > 1                      # widths differ inside the line
            used.update(ta)
    assert used == set(t for t, _ in G.SPELLED)                          # every spelling is read, as a value and as a read quality
    rows, _, n = host_equals_brute(tmp_path, native, control, 2)
    assert n == 3 and host_equals_brute(tmp_path, native_twin, control_twin, 2)[0] == rows
    assert G.servable(native, control, 2) == [] and G.servable(native_twin, control_twin, 2) == []


def test_empty(tmp_path):
    pairs = G.empty_pairs()
    assert sorted(pairs) == ['all below depth', 'both empty', 'empty control', 'empty native', 'no shared key']
    for name, (native, control) in pairs.items():
        assert host_equals_brute(tmp_path, native, control, 3) == (b'', b'', 0), name
        assert G.servable(native, control, 3) == []
    native, control = pairs['no shared key']
    assert native and control and not set(G.first_contexts(native)[0]) & set(G.first_contexts(control)[0])
    native, control = pairs['all below depth']
    shared = K.brute_sites(native, control, 2)
    assert len(shared) == 3 and all(min(len(x), len(y)) == 2 for _, _, x, y in shared) and max(len(x) for _, _, x, _ in shared) == 3


def test_decline_columns_have_the_status_they_are_built_for():
    TW = _lib.TW_STATUS
    assert (TW['far_tail'], TW['all_equal'], TW['tie'], TW['unprintable']) == (4, 16, 32, 64)
    assert _lib.twosample(*G.tie_column())[0] == 32
    assert _lib.twosample(*G.print_column())[0] == 96
    assert _lib.twosample(*G.far_tail_and_tie_column())[0] == 36
    x, y = G.far_tail_column()
    assert len(x) == len(y) == 40 and _lib.twosample(x, y)[0] == 4
    assert _lib.twosample(*G.all_equal_column(40))[0] & 16


def test_combine_declines(tmp_path):
    """Per case: the statuses of every site's columns (host build), and from them the reason and line the device has to name --
    cu_tw_reason's order over the OR of a site's columns, the smallest head line among the declining sites."""
    TW = _lib.TW_STATUS

    def reason_of(st):                                                  # cu_tw_reason (mc_curcompare.inc), restated
        for bits, name in ((TW['all_equal'], 'all_equal'), (TW['bad_n'] | TW['zero_var'], 'nan'), (TW['deep'], 'depth'), (TW['far_tail'], 'far_tail'),
                           (TW['unprintable'], 'print')):
            if st & bits:
                return name
        return 'tie'
    cases = G.combine_declines()
    assert len(cases) == 7
    for name, (native, control, depth, reason, line) in cases.items():
        host_equals_brute(tmp_path, native, control, depth)
        _, order = G.first_contexts(native)
        nat_lines = native.decode().splitlines()
        declining = []
        for (chrom, pos, strand), _, x, y in K.brute_sites(native, control, depth):
            st = [_lib.twosample(np.ascontiguousarray(x[:, j]), np.ascontiguousarray(y[:, j]))[0] for j in range(x.shape[1])]
            head = min(i for i, l in enumerate(nat_lines) if l.startswith('%s\t' % chrom) and l.split('\t')[2] == pos)
            if any(st):
                declining.append((head, reason_of(int(np.bitwise_or.reduce(st))), st))
        assert declining and min(declining)[:2] == (line, reason), (name, declining)
        if name.startswith('column 2'):
            assert len(declining) == 1 and declining[0][2][:2] == [0, 0] and declining[0][2][2] != 0, (name, declining)
        if name == 'all_equal before far_tail':
            assert declining[0][2][0] & TW['all_equal'] and declining[0][2][1] == TW['far_tail']
        if ' before ' in name and 'all_equal' not in name:
            assert len(declining) == 2 and declining[0][1] != declining[1][1]
        assert G.servable(native, control, depth) != []
