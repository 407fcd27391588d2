"""compare_currents on the GPU (mcaller_amd/csrc/compare/mc_curcompare.inc, csrc/mc_curcombine.h; Device.currents_compare,
compare_currents.compare_currents_device) against the host statement: the device's bytes equal the host's, text to text and file to
file, with `reason is None` on every case that is not a decline; every decline with its reason, file and line and the host's output or
error behind it."""
import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import compare_currents as CC
from tests import currents_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def device_makes_it(dev, tmp_path, native, control, depth=15, fdr=False, by=None, threshold=2.0, what=''):
    """The device's rows and bed equal the host statement's, from the texts and from the files; -> (rows, bed, n_sites)."""
    p1, p2 = K.files(tmp_path, native, control)
    want, want_bed, n, n_sig = CC._rows(p1, p2, depth, fdr, by or 'mwu', threshold, by is not None)
    blob, bed, n_sites, sig, reason = dev.currents_compare(text1=native, text2=control, depth=depth, fdr=fdr, by=by, threshold=threshold)
    assert reason is None, (what, reason)
    assert blob == want and (n_sites, sig) == (n, n_sig) and bed == (want_bed or b''), what
    out, sig_bed = str(tmp_path / 'out.tsv'), str(tmp_path / 'sig.bed')
    assert CC.compare_currents_device(p1, p2, out=out, depth=depth, fdr=fdr, sig_bed=sig_bed if by else None, by=by or 'mwu', threshold=threshold) == n
    assert CC.last_compare == dict(by='device', reason=None, n_sites=n, n_sig=n_sig), (what, CC.last_compare)
    assert open(out, 'rb').read() == want and (by is None or open(sig_bed, 'rb').read() == want_bed), what
    return want, want_bed, n


def host_does_it(dev, tmp_path, native, control, reason, file, line, error=None, **kw):
    """The device declines with the reason, file and line, and the host statement's output or error stands behind it."""
    p1, p2 = K.files(tmp_path, native, control)
    out = str(tmp_path / 'out.tsv')
    if error is not None:
        with pytest.raises(ValueError, match=error):
            CC.compare_currents_device(p1, p2, out=out, **kw)
    else:
        want, n = CC.compare_rows(p1, p2, kw.get('depth', 15), kw.get('fdr', False))
        assert CC.compare_currents_device(p1, p2, out=out, **kw) == n
        assert CC.last_compare['by'] == 'host' and CC.last_compare['reason'], CC.last_compare
        assert open(out, 'rb').read() == want
    st = dev.currents_compare_last_stats()
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE[reason], file, line), st


def test_rank_kernel_edges(dev, tmp_path):
    """Pooled sizes at the edges of the wave kernel (64) and of the two workgroup instances (512, 8192), two columns each."""
    native, control = K.depth_pair([4, 63, 64, 65, 512, 513, 8191, 8192])
    _, _, n = device_makes_it(dev, tmp_path, native, control, depth=2, what='rank edges')
    st = dev.currents_compare_last_stats()
    assert n == 8 and (st['n_rank_small'], st['n_rank_large'], st['deepest_site'], st['n_columns']) == (3 * 2, 5 * 2, 8192, 2), st


def test_depth_cap_declines_with_file_and_line(dev, tmp_path):
    native, control = K.depth_pair([6, 8193, 8])
    host_does_it(dev, tmp_path, native, control, 'depth', 1, 3, depth=2)
    assert 'native' in CC.last_compare['reason'] and 'line 4' in CC.last_compare['reason']


@pytest.mark.parametrize('endings', ['both', 'native lacks', 'control lacks', 'both lack'])
def test_staging_tiles_text_boundary_and_line_endings(dev, tmp_path, endings):
    """About 420 lines a file, the sites' rows shuffled together: every site's rows lie in several 256-line tiles, and the tile that
    holds the end of the native text holds the control's first rows; a last line without its newline in either file."""
    native, control = K.seeded_pair(60, 5, 9, seed=29)
    assert 256 < native.count(b'\n') < 512 and native.count(b'\n') % 256 not in (0, 255)
    if endings in ('native lacks', 'both lack'):
        native = native[:-1]
    if endings in ('control lacks', 'both lack'):
        control = control[:-1]
    assert device_makes_it(dev, tmp_path, native, control, depth=5, fdr=True, by='t', threshold=1.0, what=endings)[2] == 60


def test_row_order_decides_the_means_and_the_device_follows(dev, tmp_path):
    """0.1 + 0.2 + 0.3 is not 0.3 + 0.2 + 0.1 in fp64: with the control's column at 0.2 the means are equal in one order of the native
    rows (t = 0.0) and differ in the other (t = -0.0 after rounding).  The site's rows lie in three tiles among other sites' rows."""
    assert np.mean(np.asarray([0.1, 0.2, 0.3])) != np.mean(np.asarray([0.3, 0.2, 0.1])) and np.mean(np.asarray([0.1, 0.2, 0.3])) == np.mean(np.asarray([0.2, 0.2, 0.2]))
    filler_n, filler_c = K.seeded_pair(170, 3, 5, seed=31, c=2)
    fn, fc = filler_n.decode().splitlines(True), filler_c.decode().splitlines(True)
    assert len(fn) > 600
    mine = [K.row('chrQ', 77, '-', [v, w], read='q%d' % i) for i, (v, w) in enumerate([(0.1, 0.7), (0.2, -0.4), (0.3, 0.1)])]
    theirs = [K.row('chrQ', 77, '-', [0.2, w], read='r%d' % i) for i, w in enumerate([0.3, 0.9, -0.2])]
    outs = []
    for order in ((0, 1, 2), (2, 1, 0)):
        lines = list(fn)
        for at, k in zip((10, 300, 600), order):
            lines.insert(at, mine[k])
        native, control = ''.join(lines).encode(), ''.join(fc[:100] + theirs + fc[100:]).encode()
        rows, _, n = device_makes_it(dev, tmp_path, native, control, depth=3, what='order %s' % (order,))
        site = [r.split('\t') for r in rows.decode().splitlines() if r.startswith('chrQ\t')]
        assert len(site) == 1 and n == 171
        outs.append(site[0][7])
    assert outs == ['0.0', '-0.0']


def test_hash_collisions(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', 'f')
    native, control = K.seeded_pair(40, 3, 6, seed=37, c=3)
    assert device_makes_it(dev, tmp_path, native, control, depth=3, what='sixteen chains')[2] == 40
    assert dev.currents_compare_last_stats()['longest_probe'] > 2


def test_fdr_across_a_block(dev, tmp_path):
    """600 sites of depth 2 + 2: the radix sort and the two-level minimum cross a block of 256."""
    native, control = K.seeded_pair(600, 2, 2, seed=41, c=2, shuffle=False, planted=3)
    assert device_makes_it(dev, tmp_path, native, control, depth=2, fdr=True, by='rs', threshold=0.1, what='fdr')[2] == 600
    assert dev.currents_compare_last_stats()['n_fdr_columns'] == 4


def test_sig_bed_at_the_threshold(dev, tmp_path):
    native, control = K.seeded_pair(30, 6, 10, seed=43, planted=2)
    p1, p2 = K.files(tmp_path, native, control)
    rows = [r.split('\t') for r in CC.compare_rows(p1, p2, 6)[0].decode().splitlines()]
    printed = sorted(set(float(r[7 + K.C6 + 2]) for r in rows))
    assert len(printed) >= 3
    at = printed[len(printed) // 2]                                    # a row prints exactly the threshold, others lie on both sides
    _, bed, _ = device_makes_it(dev, tmp_path, native, control, depth=6, by='t', threshold=at, what='threshold')
    got = [float(l.split('\t')[4]) for l in bed.decode().splitlines()]
    assert min(got) == at and len(got) == sum(float(r[7 + K.C6 + 2]) >= at for r in rows) < len(rows)


def test_every_new_decline_reason(dev, tmp_path):
    native, control = K.seeded_pair(3, 3, 4, seed=47, c=2, shuffle=False)
    a, b = native.decode(), control.decode()
    good = K.row('chr1', 100, '+', [0.25, 0.5])
    n1 = a.count('\n')
    cases = [('cur_fields', a + 'chr1\tr\t10\tGATC\t0.1,0.2,9.0\t+\n', b, 1, n1, 'line %d: 6 tab-separated fields' % (n1 + 1)),
             ('cur_fields', a, good.rstrip('\n') + '\tx\ty\n' + b, 2, 0, 'control.diffs.6 line 1: 9 tab-separated fields'),
             ('cur_values', a + K.row('chr1', 100, '+', [0.25, 0.5, 0.75]), b, 1, n1, 'line %d: 4 values, 3 are expected' % (n1 + 1)),
             ('cur_values', a, b + K.row('chr1', 100, '+', [0.25]), 2, b.count('\n'), '2 values, 3 are expected'),
             ('cur_pos', a + good.replace('\t100\t', '\t1o0\t'), b, 1, n1, 'a position that is no integer'),
             ('cur_pos', a, b + good.replace('\t100\t', '\t 100\t'), 2, b.count('\n'), None),      # int() takes it: the host does the file
             ('cur_pos', a + good.replace('\t100\t', '\t0100\t'), b, 1, n1, None),
             ('number', a + good.replace('9.5', 'inf'), b, 1, n1, None),                             # the read quality is parsed, not tested
             ('number', a, b + good.replace('0.25', '0.2_5'), 2, b.count('\n'), None),             # float() takes it: the host does the file
             ('number', a, b + good.replace('0.25', '0.2x5'), 2, b.count('\n'), 'a value that is no number'),
             ('control', a + good.replace('GATCM', 'GA\x01CM'), b, 1, n1, None)]
    for reason, native, control, file, line, error in cases:
        host_does_it(dev, tmp_path, native.encode(), control.encode(), reason, file, line, error, depth=3)
    # SciPy's nan sites: a column with zero pooled variance in both samples, a column all equal
    x, y = [[0.5, 0.1], [0.5, 0.3], [0.5, 0.2]], [[0.75, 0.2], [0.75, 0.4], [0.75, 0.9]]
    nat = a + ''.join(K.site_lines('chrN', 5, '+', x, 'n'))
    con = b + ''.join(K.site_lines('chrN', 5, '+', y, 'c'))
    host_does_it(dev, tmp_path, nat.encode(), con.encode(), 'nan', 1, n1, depth=3)
    con = b + ''.join(K.site_lines('chrN', 5, '+', [[0.5, v[1]] for v in y], 'c'))
    host_does_it(dev, tmp_path, nat.encode(), con.encode(), 'all_equal', 1, n1, depth=3)


def test_table_and_memory_declines(dev, tmp_path, monkeypatch):
    native, control = K.seeded_pair(40, 3, 4, seed=53, c=2)
    monkeypatch.setenv('MCALLER_CMP_TABLE_SLOTS', '16')
    p1, p2 = K.files(tmp_path, native, control)
    assert dev.currents_compare(path1=p1, path2=p2, depth=3)[0] is None
    assert dev.currents_compare_last_stats()['decline_reason'] == _lib.CMP_DECLINE['table']
    monkeypatch.delenv('MCALLER_CMP_TABLE_SLOTS')
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', '4096')
    assert dev.currents_compare(path1=p1, path2=p2, depth=3)[0] is None
    assert dev.currents_compare_last_stats()['decline_reason'] == _lib.CMP_DECLINE['memory']
    monkeypatch.delenv('MCALLER_CMP_DEVICE_BYTES')
    assert device_makes_it(dev, tmp_path, native, control, depth=3)[2] == 40
    dev.currents_compare_release()
    assert device_makes_it(dev, tmp_path, native, control, depth=3)[2] == 40


def test_random_sites(dev, tmp_path):
    """200 seeded sites of depth 15 to 60 with six columns, every fourth with a planted shift, rows shuffled across the file."""
    native, control = K.seeded_pair(200, 15, 60, seed=59)
    _, bed, n = device_makes_it(dev, tmp_path, native, control, depth=15, fdr=True, by='mwu', threshold=2.0, what='random')
    st = dev.currents_compare_last_stats()
    assert n == 200 and st['n_rank_small'] + st['n_rank_large'] == 200 * K.C6 and st['n_rank_small'] > 0 and st['n_rank_large'] > 0
    assert 20 <= bed.count(b'\n') <= 80


def test_the_command_line_says_who_made_the_output(dev, tmp_path, capsys):
    native, control = K.seeded_pair(5, 4, 6, seed=61, c=3)
    p1, p2 = K.files(tmp_path, native, control)
    out = str(tmp_path / 'o.tsv')
    CC.main(['--native', p1, '--control', p2, '-d', '4', '-o', out, '--device'])
    assert CC.last_compare['by'] == 'device' and open(out, 'rb').read() == CC.compare_rows(p1, p2, 4)[0]
    assert 'host statement' not in capsys.readouterr().err
    open(p2, 'ab').write(b'chr1\tr\t 5\tGATC\t0.1,0.2,0.3,9.0\t+\tA\n')
    CC.main(['--native', p1, '--control', p2, '-d', '4', '-o', out, '--device'])
    assert CC.last_compare['by'] == 'host' and open(out, 'rb').read() == CC.compare_rows(p1, p2, 4)[0]
    assert 'the host statement made the output' in capsys.readouterr().err
