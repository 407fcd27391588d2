"""The record rules of a FASTQ file (mcaller_amd/csrc/mc_fastqrec.h) run on the CPU, _lib.fastq_records_host, against the plain-Python
statement read_qual.extract_read_quality_py: the same keys in the same order, every mean equal by == or both NaN, as np.float64 --
or a decline with its reason and line.  The device reader (tests/test_gpu_fastq.py) is held against both."""
import numpy as np
import pytest

from mcaller_amd import _lib
from tests import fastq_cases as F


def host_dict(text):
    keys, means, decline = _lib.fastq_records_host(text)
    assert decline is None, decline
    return keys, means, dict(zip(keys, means))


@pytest.mark.parametrize('name,text,pairs', F.LISTED, ids=[c[0] for c in F.LISTED])
def test_listed_texts(name, text, pairs):
    keys, means, got = host_dict(text)
    F.assert_pairs(keys, means, pairs, name)
    want = F.statement(text)
    F.assert_same_dict(got, want, name)
    F.assert_same_dict(got, dict((k, np.float64(v)) for k, v in pairs), name)


def test_listed_dict_order_of_duplicate_keys():
    text = dict((c[0], c[1]) for c in F.LISTED)['duplicate keys']
    _, _, got = host_dict(text)
    assert list(got.items()) == [('a', 1.0), ('b', 20.0)]


@pytest.mark.parametrize('kind', sorted(F.KINDS))
def test_random_files(kind):
    text = F.random_fastq(np.random.default_rng(7), 3000, **F.KINDS[kind])
    keys, means, got = host_dict(text)
    assert len(keys) == 3000 and means.shape == (3000,)
    assert np.isnan(means).sum() >= 30                       # (reads of length 0 are among them)
    F.assert_same_dict(got, F.statement(text), kind)


@pytest.mark.parametrize('name,text,reason,line', F.DECLINES, ids=[c[0] for c in F.DECLINES])
def test_declines(name, text, reason, line):
    keys, means, decline = _lib.fastq_records_host(text)
    assert keys is None and means is None
    assert (decline['reason'], decline['line']) == (reason, line), decline
    assert 'declines' in decline['text'] and '(line %d)' % (line + 1) in decline['text']


def test_the_statement_reads_what_a_blank_line_declines():
    text = dict((c[0], c[1]) for c in F.DECLINES)['blank line before a title']
    assert F.statement(text) == {'r': np.float64(40.0)}


def test_word_tests_agree_with_the_byte_rules():
    """Every decline of a single byte at every place of a 16-byte group, in front of a newline and not: the word-parallel tests of the
    device build see four bytes at a time, the host build one -- on the CPU only the latter runs, so this pins the rule itself."""
    for bad, reason in ((0x80, 'high_byte'), (0xff, 'high_byte'), (0x00, 'control'), (0x1f, 'control'), (0x7f, 'control'), (0x0d, 'lone_cr')):
        for at in range(16):
            seq = bytearray(b'ACGTACGTACGTACGT')
            seq[at] = bad
            text = b'@r\n' + bytes(seq) + b'\n+\n' + b'I' * 16 + b'\n'
            _, _, decline = _lib.fastq_records_host(text)
            want = (F.D[reason], 1)
            if bad == 0x0d and at == 15:                         # (a line break: the sequence line is one byte shorter)
                want = (F.D['length'], 3)
            assert decline is not None and (decline['reason'], decline['line']) == want, (bad, at, decline)
