"""Two --vo BED files compared per site on the GPU (mcaller_amd/csrc/compare/mc_bedcompare.hip; Device.bed_compare,
compare_genomes.compare_by_position_device) against the host statement (compare_genomes.compare_by_position, SciPy): the same
bytes file to file and text to text, made by the device wherever tests/test_twosample.py has shown the sites to be vouched for;
every decline with its reason, file and line, and the host's output or error behind it.  mc_twosample_device against mc_twosample.
(MC_CMP_DECLINE_ROWS needs 2^31 lines: not run here.)"""
import os

import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import compare_genomes as CG
from tests import gpu_compare_cases as GC
from tests import twosample_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def files(tmp_path, t1, t2):
    p1, p2 = str(tmp_path / 'a.bed'), str(tmp_path / 'b.bed')
    open(p1, 'wb').write(t1)
    open(p2, 'wb').write(t2)
    return p1, p2


def host(p1, p2):
    """-> the host statement's bytes and site count, or the exception it raises."""
    try:
        return CG.compare_rows(p1, p2)
    except Exception as e:                        # noqa: BLE001 (whatever the statement raises is the expectation)
        return e


def device_makes_it(dev, tmp_path, t1, t2, what=''):
    """The device's bytes, text to text and file to file, equal the host statement's -> the stats of the file call."""
    p1, p2 = files(tmp_path, t1, t2)
    want, n = host(p1, p2)
    blob, n_sites, reason = dev.bed_compare(text1=t1, text2=t2)
    assert reason is None, (what, reason, dev.bed_compare_last_stats())
    assert blob == want and n_sites == n, what
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(p1, p2, out=out) == n
    assert CG.last_compare == dict(by='device', reason=None, n_sites=n), what
    assert open(out, 'rb').read() == want, what
    st = dev.bed_compare_last_stats()
    assert st['decline_reason'] == 0 and st['decline_line'] == -1 and st['decline_file'] == 0 and st['n_sites'] == n
    assert st['n_out_bytes'] == len(want)
    return st


def test_wave_and_workgroup_edges(dev, tmp_path):
    """Pooled sizes 2 + 1, 63, 64, 65 (the wave kernel's edge), 512, 513 (between the workgroup kernel's two instances) and 8191,
    8192 (its cap); a site whose rank-sum z is an exact rounding tie, a site with equal means."""
    t1, t2 = GC.edge_pair()
    st = device_makes_it(dev, tmp_path, t1, t2, 'edges')
    assert st['n_rank_small'] == 8 and st['n_rank_large'] == 10 and st['deepest_site'] == 8192


def test_one_value_too_deep_declines(dev, tmp_path):
    t1, t2 = GC.deep_pair()
    p1, p2 = files(tmp_path, t1, t2)
    want, n = host(p1, p2)
    blob, n_sites, reason = dev.bed_compare(path1=p1, path2=p2)
    st = dev.bed_compare_last_stats()
    assert blob is None and 'more than 8192' in reason
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['depth'], 1, 1)
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(p1, p2, out=out) == n == 3
    assert CG.last_compare['by'] == 'host' and '8192' in CG.last_compare['reason']
    assert open(out, 'rb').read() == want


def test_sites_across_tiles(dev, tmp_path):
    t1, t2 = GC.straddle_pair()
    assert len(t1) > 3 * 16384 and t1.count(b'\n') > 1024
    st = device_makes_it(dev, tmp_path, t1, t2, 'straddle')
    assert 256 < st['n_sites'] < t1.count(b'\n')


def test_keys_that_differ_in_one_place(dev, tmp_path):
    t1, t2 = GC.key_pair()
    st = device_makes_it(dev, tmp_path, t1, t2, 'keys')
    assert st['n_sites'] == 8


def test_long_probe_chains(dev, tmp_path, monkeypatch):
    """Sixteen hash values for all keys and no tag: the byte comparison decides."""
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', 'f')
    t1, t2 = GC.small_pair()
    st = device_makes_it(dev, tmp_path, t1, t2, 'hash mask')
    assert st['longest_probe'] >= 3
    t1, t2 = GC.key_pair()
    device_makes_it(dev, tmp_path, t1, t2, 'hash mask, keys')


@pytest.mark.parametrize('file', [1, 2])
def test_duplicate_at_the_end_of_a_probe_chain(dev, monkeypatch, file):
    """Forty keys in sixteen hash values (one cluster of taken slots), one of them once more as the file's last line: the later line
    of the pair is named, as in duplicate_1 / duplicate_2 without the mask."""
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', 'f')
    t1, t2 = GC.small_pair()
    assert t1.count(b'\n') == t2.count(b'\n') == 40
    if file == 1:
        t1 += t1.splitlines(True)[3]
    else:
        t2 += t2.splitlines(True)[17]
    blob, n_sites, why = dev.bed_compare(text1=t1, text2=t2)
    st = dev.bed_compare_last_stats()
    assert blob is None and n_sites == 0 and '(bed%d)' % file in why and '(line 41)' in why
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['duplicate'], file, 40)


def test_table_forced_too_small_declines(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_CMP_TABLE_SLOTS', '8')
    t1, t2 = GC.small_pair()
    blob, n_sites, reason = dev.bed_compare(text1=t1, text2=t2)
    st = dev.bed_compare_last_stats()
    assert blob is None and 'table is full' in reason and st['decline_reason'] == _lib.CMP_DECLINE['table']
    p1, p2 = files(tmp_path, t1, t2)
    out = str(tmp_path / 'out.tsv')
    CG.compare_by_position_device(p1, p2, out=out)
    assert CG.last_compare['by'] == 'host' and open(out, 'rb').read() == host(p1, p2)[0]


def test_too_little_device_memory_declines(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', '1000')
    t1, t2 = GC.small_pair()
    blob, n_sites, reason = dev.bed_compare(text1=t1, text2=t2)
    st = dev.bed_compare_last_stats()
    assert blob is None and 'do not fit' in reason and '(line' not in reason
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['memory'], 0, -1)
    p1, p2 = files(tmp_path, t1, t2)
    out = str(tmp_path / 'out.tsv')
    CG.compare_by_position_device(p1, p2, out=out)
    assert CG.last_compare['by'] == 'host' and open(out, 'rb').read() == host(p1, p2)[0]
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', str(1 << 30))
    device_makes_it(dev, tmp_path, t1, t2, 'memory enough')


def test_many_stage_blocks(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_TEXT_STAGE_BYTES', '256')
    t1, t2 = GC.small_pair()
    assert len(t1) > 10 * 256 and len(t2) > 10 * 256
    device_makes_it(dev, tmp_path, t1, t2, 'stage blocks')


@pytest.mark.parametrize('cut1,cut2', [(True, False), (False, True), (True, True)])
def test_last_line_without_newline(dev, tmp_path, cut1, cut2):
    t1, t2 = GC.small_pair()
    device_makes_it(dev, tmp_path, t1[:-1] if cut1 else t1, t2[:-1] if cut2 else t2, 'no newline')


def test_no_shared_key_and_empty_files(dev, tmp_path):
    t1, t2 = GC.small_pair()
    other = t2.replace(b'chr1\t', b'chr2\t')
    for a, b in ((t1, other), (t1, b''), (b'', t2), (b'', b'')):
        st = device_makes_it(dev, tmp_path, a, b, 'nothing shared')
        assert st['n_sites'] == 0 and st['n_out_bytes'] == 0


DECLINES = GC.declines()


@pytest.mark.parametrize('name', sorted(DECLINES))
def test_every_decline(dev, tmp_path, name):
    t1, t2, reason, file, line, error = DECLINES[name]
    blob, n_sites, why = dev.bed_compare(text1=t1, text2=t2)
    st = dev.bed_compare_last_stats()
    print(name, why, st)
    assert blob is None and n_sites == 0 and why
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE[reason], file, line)
    assert '(bed%d)' % file in why and '(line %d)' % (line + 1) in why
    p1, p2 = files(tmp_path, t1, t2)
    want = host(p1, p2)
    out = str(tmp_path / 'out.tsv')
    if isinstance(want, Exception):
        assert error is None or isinstance(want, error)
        with pytest.raises(type(want)):
            CG.compare_by_position_device(p1, p2, out=out)
    else:
        assert error is None
        assert CG.compare_by_position_device(p1, p2, out=out) == want[1]
        assert CG.last_compare['by'] == 'host' and CG.last_compare['reason'] == why
        assert open(out, 'rb').read() == want[0]


def test_cli_device(dev, tmp_path, capfd):
    t1, t2 = GC.small_pair()
    p1, p2 = files(tmp_path, t1, t2)
    CG.main(['--bed1', p1, '--bed2', p2, '--device'])
    assert capfd.readouterr().out.encode() == host(p1, p2)[0]
    assert CG.last_compare['by'] == 'device'


def test_twosample_device_against_host_build(dev):
    """The CPU test's sample set through the rank kernels and kc_finish: integers, U and D bit for bit, the status the same, the
    device's bounds the host build's, every vouched value equal, every other one within a thousandth and the two bounds."""
    cases = T.seeded() + T.seeded([(256, 256), (256, 257)] + T.HOST_ONLY_SIZES[:1]) + [('exact tie',) + GC.exact_tie_site(), ('equal means',) + GC.equal_means_site()] + [(k, np.asarray(v[0], dtype=float), np.asarray(v[1], dtype=float))
                                                           for k, v in sorted(T.DEGENERATE.items())]
    st, out, bound = dev.twosample([c[1] for c in cases], [c[2] for c in cases])
    for i, (name, x, y) in enumerate(cases):
        hs, ho, hb = _lib.twosample(x, y)
        if len(x) + len(y) > 8192:
            assert st[i] == _lib.TW_STATUS['deep'], name
            continue
        print(name, st[i], hs, out[i].tolist(), ho.tolist())
        assert st[i] == hs, (name, st[i], hs)
        assert out[i, 0].tobytes() == ho[0].tobytes() and out[i, 4].tobytes() == ho[4].tobytes(), name
        if np.isnan(ho[1]) or hs & _lib.TW_STATUS['far_tail']:      # (no value to bound: SciPy's nan, or inf on both sides)
            continue
        # the stated bounds: the device's own equal the host build's up to the moments' last bits, and none is wide enough to
        # move a value by a thousandth
        assert np.all(np.isfinite(bound[i])) and np.all(bound[i] >= 0.0), name
        assert np.allclose(bound[i, :5], hb[:5], rtol=1e-6, atol=1e-300), (name, bound[i].tolist(), hb.tolist())
        # a tail's bound is the difference of two evaluations plus the function term FN * (1 - log10 p): the device's evaluations
        # are within that term of the host's each, so the two bounds differ by twice the host's at the most
        assert np.all(np.abs(bound[i, 5:] - hb[5:]) <= 2.0 * hb[5:]), (name, bound[i].tolist(), hb.tolist())
        assert bound[i, 1] == 0.0 and bound[i, 2] == 0.0, name                 # z_mwu, z_rs: the host's bits
        if hs == 0:
            assert out[i].tobytes() == ho.tobytes(), name
        else:
            with np.errstate(invalid='ignore'):             # (a far tail: inf on both sides)
                # values rounded to thousandths from unrounded ones at most the two bounds apart
                assert np.all((out[i] == ho) | (np.abs(out[i] - ho) <= 0.001 + bound[i] + hb + 1e-12)), name
