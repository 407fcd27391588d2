"""The read qualities of a FASTQ file made on the GPU (mcaller_amd/csrc/fastq/mc_fastqual.hip; Device.fastq_qualities,
read_qual.extract_read_quality_device) against the record rules on the CPU (_lib.fastq_records_host) and the plain-Python statement
(read_qual.extract_read_quality_py): keys in order, means bit for bit.  None of the files the statement reads here may be declined,
and what is declined is declined with the host build's reason and line."""
import contextlib
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from mcaller_amd import _lib
from tests import fastq_cases as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

TILE = 16384                      # bytes a workgroup of the stream kernels takes


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def device_equals_host(dev, text, what='', statement=True, **how):
    """-> (keys, means) of the device, equal to the host build's and (statement=True) giving the Python statement's dict."""
    keys, means, reason = dev.fastq_qualities(**(how or dict(text=text)))
    assert reason is None, (what, reason)
    hk, hm, decline = _lib.fastq_records_host(text)
    assert decline is None, (what, decline)
    assert keys == hk, what
    assert means.dtype == np.float64 and means.tobytes() == hm.tobytes(), what          # (NaNs too: both are the same quiet NaN or this fails)
    if statement:
        F.assert_same_dict(dict(zip(keys, means)), F.statement(text), what)
    return keys, means


@pytest.mark.parametrize('name,text,pairs', F.LISTED, ids=[c[0] for c in F.LISTED])
def test_listed_texts(dev, name, text, pairs):
    keys, means = device_equals_host(dev, text, name)
    F.assert_pairs(keys, means, pairs, name)
    st = dev.fastq_qualities_last_stats()
    assert st['n_records'] == len(pairs) and st['decline_reason'] == 0 and st['decline_line'] == -1


@pytest.mark.parametrize('kind', sorted(F.KINDS))
def test_random_files(dev, kind):
    text = F.random_fastq(np.random.default_rng(7), 3000, **F.KINDS[kind])
    keys, _ = device_equals_host(dev, text, kind)
    assert len(keys) == 3000


@pytest.mark.parametrize('name,text,reason,line', F.DECLINES, ids=[c[0] for c in F.DECLINES])
def test_declines(dev, name, text, reason, line):
    keys, means, why = dev.fastq_qualities(text=text)
    st = dev.fastq_qualities_last_stats()
    assert keys is None and means is None and 'declines' in why
    assert (st['decline_reason'], st['decline_line']) == (reason, line), (st, why)
    _, _, decline = _lib.fastq_records_host(text)
    assert decline['text'] == why


def edge_text(piece, fill, rng):
    """One record per (length, alignment of the quality line's first byte): the title's length puts the line where it is wanted."""
    lengths = [0, 1, 15, 16, 17, 63, 64, 65, piece - 1, piece, piece + 1, 3 * piece + 5, 70001]
    parts, at, want = [], 0, []
    for n in lengths:
        for align in range(16):
            head = '@e%d_%d ' % (n, align)
            rest = len('\n') + n + len('\n+\n')                        # between the title's last byte and the quality line's first
            pad = (align - (at + len(head) + rest)) % 16
            if fill == 'random':
                qual = rng.integers(33, 127, n, dtype=np.uint8).tobytes()
            else:
                qual = fill.encode('ascii') * n
            rec = head.encode('ascii') + b'p' * pad + b'\n' + b'A' * n + b'\n+\n' + qual + b'\n'
            assert (at + len(rec) - len(qual) - 1) % 16 == align
            parts.append(rec)
            at += len(rec)
            want.append(('e%d' % n, n, sum(qual)))
    return b''.join(parts), want


@pytest.mark.parametrize('fill', ['random', '~', '!'])
def test_quality_lines_at_every_edge_of_the_sum(dev, fill):
    dev.fastq_qualities(text=b'@r\nA\n+\nI\n')
    piece = dev.fastq_qualities_last_stats()['piece_bytes']
    assert piece >= 64 and piece % 16 == 0
    text, want = edge_text(piece, fill, np.random.default_rng(3))
    keys, means = device_equals_host(dev, text, fill)
    assert keys == [k for k, _, _ in want]
    for got, (key, n, total) in zip(means, want):              # said once more without either reader: exact integers, one division
        assert (np.isnan(got) if n == 0 else got == np.float64(total - 33 * n) / np.float64(n)), (key, n)
    st = dev.fastq_qualities_last_stats()
    assert st['n_pieces'] == sum(-(-n // piece) for _, n, _ in want)


@pytest.mark.parametrize('crlf', [False, True], ids=['plain', 'crlf'])
@pytest.mark.parametrize('final_newline', [True, False], ids=['newline', 'no_newline'])
def test_record_counts(dev, crlf, final_newline):
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        text = F.random_fastq(np.random.default_rng(n), n, crlf=crlf)
        if not final_newline:
            text = text[:-2] if crlf else text[:-1]
        keys, _ = device_equals_host(dev, text, (n, crlf, final_newline))
        assert len(keys) == n


@pytest.mark.parametrize('at', [3, 4, 15, 16, 63, 64, TILE - 1, TILE, 2 * TILE - 1])
def test_line_break_across_a_word_a_lane_and_a_tile(dev, at):
    """'\\r' at byte `at` with its '\\n' behind it -- the last byte of a word, of a lane's 64 bytes, of a 16 KB tile -- is a line break;
    with another byte behind it the text is declined."""
    title = b'@r ' + b'x' * (at - 3)
    assert len(title) == at
    keys, means = device_equals_host(dev, title + b'\r\nAC\n+\nII\n', at)
    assert keys == ['r'] and means[0] == 40.0
    bad = title + b'\rA\nAC\n+\nII\n'
    keys, means, why = dev.fastq_qualities(text=bad)
    st = dev.fastq_qualities_last_stats()
    assert keys is None and (st['decline_reason'], st['decline_line']) == (F.D['lone_cr'], 0), (st, why)
    assert _lib.fastq_records_host(bad)[2]['text'] == why
    # ... and as the very last byte of a text that fills its tile
    end = b'@r\n' + b'A' * (at - 3) + b'\r'
    keys, means, why = dev.fastq_qualities(text=end)
    assert keys is None and dev.fastq_qualities_last_stats()['decline_reason'] == F.D['lone_cr']


@pytest.fixture(scope='module')
def long_read():
    n = 48 * 10 ** 6
    return b'@long_read:1\n' + b'A' * n + b'\n+\n' + b'~' * n + b'\n'


def test_one_read_whose_sums_pass_32_bits(dev, long_read):
    n = 48 * 10 ** 6
    assert 126 * n > 2 ** 32 and 93 * n > 2 ** 32
    keys, means = device_equals_host(dev, long_read, 'long read')
    assert keys == ['long'] and means[0] == 93.0
    st = dev.fastq_qualities_last_stats()
    assert st['n_pieces'] == -(-n // st['piece_bytes']) and st['n_lines'] == 4


def test_a_file_read_in_blocks_equals_its_text(dev, long_read, tmp_path):
    path = str(tmp_path / 'long.fastq')
    text = long_read + F.random_fastq(np.random.default_rng(2), 500)
    assert len(text) >= 64 << 20
    with open(path, 'wb') as f:
        f.write(text)
    a = dev.fastq_qualities(text=text)
    keys, means = device_equals_host(dev, text, 'file', statement=False, path=path)
    assert a[2] is None and a[0] == keys and a[1].tobytes() == means.tobytes() and len(keys) == 501
    st = dev.fastq_qualities_last_stats()
    assert st['n_bytes'] == len(text) and st['ms_read'] > 0
    dev.fastq_qualities_release()
    # then a small one on the same context: nothing of the large one is left
    keys, means = device_equals_host(dev, b'@s\nAC\n+\nI5\n', 'small behind large')
    assert keys == ['s'] and means.tolist() == [30.0]


def test_two_calls_in_a_row(dev):
    from tests._fastq_pair_worker import pair
    pair(dev)


def test_two_calls_in_a_row_with_poisoned_allocations():
    env = dict(os.environ, MCALLER_POISON='1', PYTHONPATH=H.REPO)
    done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_fastq_pair_worker.py')], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0 and b'pair ok' in done.stdout, done.stdout.decode('utf-8', 'replace')[-2000:]


# ---- the command line ----
@pytest.fixture(scope='module')
def td(tmp_path_factory):
    return H.testdata_paths(str(tmp_path_factory.mktemp('testdata')))


def run_cli(td, d, fastq):
    from mcaller_amd import mCaller
    os.makedirs(d, exist_ok=True)
    tsv = os.path.join(d, 'masonread1.eventalign.tsv')
    shutil.copy(td['tsv'], tsv)
    model = os.path.join(H.MODELS, 'r95_twobase_model_NN_6_m6A.npz')
    with contextlib.redirect_stdout(io.StringIO()):
        mCaller.main(['-m', 'GATC', '-r', td['fasta'], '-e', tsv, '-f', fastq, '-d', model])
    return open(os.path.join(d, 'masonread1.eventalign.diffs.6'), 'rb').read()


@pytest.fixture(scope='module')
def without_the_knob(td, tmp_path_factory):
    from mcaller_amd import read_qual
    assert os.environ.get('MCALLER_FASTQ_DEVICE', '0') != '1'
    rows = run_cli(td, str(tmp_path_factory.mktemp('host')), td['fastq'])
    assert read_qual.last_read['by'] == 'host' and len(rows) > 1000
    return rows


def test_cli_with_the_device_reader(td, tmp_path, monkeypatch, without_the_knob):
    from mcaller_amd import read_qual
    monkeypatch.setenv('MCALLER_FASTQ_DEVICE', '1')
    read_qual.last_read = None
    rows = run_cli(td, str(tmp_path / 'device'), td['fastq'])
    assert read_qual.last_read['by'] == 'device' and read_qual.last_read['reason'] is None and read_qual.last_read['n_records'] > 0
    assert rows == without_the_knob


def test_cli_with_a_blank_line_between_records(td, tmp_path, monkeypatch, without_the_knob):
    from mcaller_amd import read_qual
    fastq = str(tmp_path / 'blank.fastq')
    with open(fastq, 'wb') as f:                             # (the committed file holds one read; the second is in no row of the eventalign file)
        f.write(open(td['fastq'], 'rb').read().rstrip(b'\n') + b'\n\n@another_read:1\nAC\n+\nII\n')
    monkeypatch.setenv('MCALLER_FASTQ_DEVICE', '1')
    read_qual.last_read = None
    rows = run_cli(td, str(tmp_path / 'blank'), fastq)
    assert read_qual.last_read['by'] == 'host' and 'title line' in read_qual.last_read['reason']
    assert rows == without_the_knob


def test_cli_with_a_gz_path(td, tmp_path, monkeypatch, without_the_knob):
    import gzip
    from mcaller_amd import read_qual
    fastq = str(tmp_path / 'reads.fastq.gz')
    with gzip.open(fastq, 'wb') as f:
        f.write(open(td['fastq'], 'rb').read())
    monkeypatch.setenv('MCALLER_FASTQ_DEVICE', '1')
    read_qual.last_read = None
    rows = run_cli(td, str(tmp_path / 'gz'), fastq)
    assert read_qual.last_read['by'] == 'host' and 'gzip' in read_qual.last_read['reason']
    assert rows == without_the_knob
