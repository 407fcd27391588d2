"""The merge behind `-t N` on the GPU (csrc/merge/mc_rowmerge.hip; Device.merge_rows, mCaller.merge_like_sort_uniq_device) against
mCaller.merge_like_sort_uniq on the same files: the smallest shapes at which the kernels can go wrong (tests/merge_files.py),
300 seeded random files, the declines, and `mCaller -t 4` itself."""
import glob
import os

import pytest

from tests import helpers as H
from tests import merge_files as MF

pytestmark = pytest.mark.gpu

EDGE = MF.edge_cases()
DECLINE = MF.decline_cases()


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def device_merge(parts, directory, monkeypatch, want_by):
    """The parts through merge_like_sort_uniq_device, file to file -> the bytes written; the part files are gone and no
    temporary output is left."""
    from mcaller_amd import mCaller
    monkeypatch.setenv('MCALLER_MERGE_DEVICE', '1')
    paths = MF.write_parts(parts, directory)
    out = os.path.join(str(directory), 'rows.merged')
    mCaller.merge_like_sort_uniq_device(paths, out)
    assert mCaller.last_merge['by'] == want_by, mCaller.last_merge
    assert not any(os.path.exists(p) for p in paths)
    assert sorted(os.listdir(str(directory))) == ['rows.merged']
    with open(out, 'rb') as fh:
        return fh.read()


@pytest.mark.parametrize('name', sorted(EDGE))
def test_edge_files_merge_to_the_host_bytes(name, dev, tmp_path, monkeypatch):
    from mcaller_amd import mCaller
    parts = EDGE[name]
    want = MF.host_merge(parts, tmp_path)
    got = device_merge(parts, tmp_path, monkeypatch, 'device')
    assert got == want
    assert mCaller.last_merge['n_written'] == want.count(b'\n') and mCaller.last_merge['n_lines'] == b''.join(parts).count(b'\n')
    # the text entry point on the parts one behind the other: the same bytes
    blob, reason = dev.merge_rows(text=b''.join(parts))
    assert reason is None and blob == want
    st = dev.merge_rows_last_stats()
    assert st['decline_reason'] == 0 and st['decline_line'] == -1 and st['n_lines_out'] == want.count(b'\n')
    assert st['n_out_bytes'] == len(want) and st['n_bytes'] == sum(len(p) for p in parts)


def test_the_stats_say_how_the_sort_went(dev):
    blob, reason = dev.merge_rows(text=EDGE['one_read_5000'][0])
    st = dev.merge_rows_last_stats()
    assert reason is None and st['n_lines'] == 5000 == st['n_lines_out'] == st['n_tied_after_key']
    # one read: the rows agree up to the position, byte 46 on -- two rounds for the key, then one per 8 bytes of the line
    assert 2 + 6 <= st['n_rounds'] <= 2 + 9 and st['n_passes'] >= 2 and 2 <= st['largest_compared'] <= MF.SMALL
    assert st['kernel_bytes'] > 3 * st['n_bytes'] and st['ms_kernels'] > 0
    blob, reason = dev.merge_rows(text=EDGE['two_equal_for_4000'][0])
    st = dev.merge_rows_last_stats()
    assert reason is None and st['n_rounds'] == 2 and st['largest_compared'] == 2      # finished by comparison, not by 500 rounds


@pytest.mark.parametrize('first', (0, 100, 200))
def test_random_files_merge_to_the_host_bytes(first, dev, tmp_path, monkeypatch):
    for seed in range(first, first + 100):
        parts = MF.random_file(seed)
        d = tmp_path / str(seed)
        d.mkdir()
        want = MF.host_merge(parts, d)
        if seed % 10 == 0:                                  # file to file ...
            got = device_merge(parts, d, monkeypatch, 'device')
        else:                                               # ... and the text entry point
            got, reason = dev.merge_rows(text=b''.join(parts))
            assert reason is None, (seed, reason)
        assert got == want, seed


@pytest.mark.parametrize('name', sorted(DECLINE))
def test_declines_name_reason_and_line_and_the_host_does_the_files(name, dev, tmp_path, monkeypatch):
    from mcaller_amd import _lib, mCaller
    parts, reason, line = DECLINE[name]
    paths = MF.write_parts(parts, tmp_path, stem='direct')
    out = str(tmp_path / 'direct.merged')
    n, why = dev.merge_rows(paths=paths, out_path=out)
    st = dev.merge_rows_last_stats()
    assert n is None and why and 'declines' in why
    assert st['decline_reason'] == _lib.MERGE_DECLINE[reason] and st['decline_line'] == line and st['decline_file'] == 0
    assert all(os.path.exists(p) for p in paths) and not glob.glob(out + '*')       # the inputs and no output
    for p in paths:
        os.remove(p)
    if len(parts) == 1:
        blob, why = dev.merge_rows(text=parts[0])
        st = dev.merge_rows_last_stats()
        assert blob is None and st['decline_reason'] == _lib.MERGE_DECLINE[reason] and st['decline_line'] == line
    want = MF.host_merge(parts, tmp_path)
    got = device_merge(parts, tmp_path, monkeypatch, 'host')
    assert got == want and mCaller.last_merge['reason'] == why


def test_the_knob_sends_the_files_to_the_host(tmp_path, monkeypatch):
    from mcaller_amd import mCaller
    parts = EDGE['cli_host_dealt']
    want = MF.host_merge(parts, tmp_path)
    monkeypatch.setenv('MCALLER_MERGE_DEVICE', '0')
    paths = MF.write_parts(parts, tmp_path)
    out = str(tmp_path / 'rows.merged')
    mCaller.merge_like_sort_uniq_device(paths, out)
    assert open(out, 'rb').read() == want and mCaller.last_merge['by'] == 'host'
    assert not any(os.path.exists(p) for p in paths)


@pytest.mark.parametrize('knob, by', (('1', 'device'), ('0', 'host')))
def test_threads_flag_on_the_testdata(knob, by, tmp_path_factory, tmp_path, monkeypatch):
    """`mCaller -m GATC -t 4`: the bytes tests/test_gpu_cli.py expects, whoever merges."""
    from mcaller_amd import mCaller
    from tests.test_gpu_cli import run_cli
    td = H.testdata_paths(str(tmp_path_factory.mktemp('testdata')))
    monkeypatch.setenv('MCALLER_MERGE_DEVICE', knob)
    mCaller.last_merge = None
    out, _ = run_cli(td, tmp_path, ['-m', 'GATC', '-t', '4'])
    want = sorted(set(open(os.path.join(H.GOLDEN, 'ref_outputs', 'motif_GATC.diffs.6'), 'rb').read().splitlines(True)))
    assert open(out, 'rb').read() == b''.join(want)
    assert mCaller.last_merge['by'] == by
    assert not glob.glob(str(tmp_path / '*.tmp*')) and not glob.glob(str(tmp_path / '*.merging'))
