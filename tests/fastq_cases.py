"""FASTQ texts for tests/test_fastq_records.py (the record rules on the CPU) and tests/test_gpu_fastq.py (the same rules on the GPU):
texts with their expected (keys, means), a generator of random files, texts the rules decline with the reason and the 0-based line."""
import math
import os
import tempfile

import numpy as np

from mcaller_amd import _lib
from mcaller_amd.read_qual import extract_read_quality_py

NAN = float('nan')
D = _lib.FASTQ_DECLINE

# (name, text, the pairs in file order) -- every record, duplicates included; the dict is dict(zip(keys, means))
LISTED = [
    ('stripped sequence', b'@r\n ACGT\t\n+\nIIII\n', [('r', 40.0)]),
    ('key cut', b'@  r1_x:y z\nAC\n+\nI5\n', [('r1', 30.0)]),
    ('empty key', b'@:a\nA\n+\nI\n', [('', 40.0)]),
    ('trailing blank lines', b'@r\nAC\n+\nII\n\n \n\t\n', [('r', 40.0)]),
    ('no final newline', b'@r\nAC\n+\nI!', [('r', 20.0)]),
    ('empty record', b'@r\n\n+\n', [('r', NAN)]),
    ('empty record, file ends with the plus line', b'@r\n\n+', [('r', NAN)]),
    ('empty record in the middle', b'@a\nAC\n+\nII\n@b\n\n+\n\n@c\nA\n+\n5\n', [('a', 40.0), ('b', NAN), ('c', 20.0)]),
    ('crlf', b'@r\r\nAC\r\n+\r\nI~\r\n', [('r', 66.5)]),
    ('duplicate keys', b'@a_1\nA\n+\n!\n@b\nA\n+\n5\n@a:2\nA\n+\n"\n', [('a', 0.0), ('b', 20.0), ('a', 1.0)]),
    ('text behind the plus', b'@r\nAC\n+r some words\nII\n', [('r', 40.0)]),
    ('empty text', b'', []),
    ('two newlines', b'\n\n', []),
    ('blanks where bases are', b'@r\nAC\n+\n  \n', [('r', -1.0)]),
    ('tab in the title', b'@\tr:1\tx\nA\n+\nI\n', [('r', 40.0)]),
]

OK = b'@ok\nAC\n+\nII\n'
# (name, text, reason, 0-based line)
DECLINES = [
    ('blank line before a title', b'\n@r\nA\n+\nI\n', D['title'], 0),                 # (the Python statement reads this one: that is the point)
    ('blank line between records', OK + b'\n@r\nA\n+\nI\n', D['title'], 4),
    ('lone cr', b'@r\nA\rC\n+\nIII\n', D['lone_cr'], 1),
    ('cr at the end of the text', b'@r\nAC\n+\nII\r', D['lone_cr'], 3),
    ('two crs', b'@r\nAC\r\r\n+\nII\n', D['lone_cr'], 1),
    ('high byte', b'@r\xc3\xa9\nA\n+\nI\n', D['high_byte'], 0),
    ('vertical tab', b'@r\nA\n+x\x0b\nI\n', D['control'], 2),
    ('del', OK + b'@r\nA\n+\n\x7f\n', D['control'], 7),
    ('no @', OK + b'read1\nACGT\n+\nIIII\n', D['title'], 4),
    ('two sequence lines', OK + b'@read1\nACGT\nACGT\n+\nIIIIIIII\n', D['plus'], 6),
    ('short quality', OK + b'@read1\nACGT\n+\nIII\n', D['length'], 7),
    ('ends inside a record', OK + b'@read1\nACGT\n', D['plus'], 6),
    ('ends behind a title', OK + b'@read1\n', D['plus'], 6),
    ('no id', b'@ \nA\n+\nI\n', D['empty_id'], 0),
    ('bare @', b'@\nA\n+\nI\n', D['empty_id'], 0),
    ('quality missing', b'@r\nAC\n+\n', D['length'], 3),
    ('two offending lines', b'@r\nAC\n+\nI\n@s\nA\n-\nI\x01\n', D['length'], 3),
    ('a byte in front of a record fault', b'@r\nA\x01\n+\nI\n@s\nA\n-\nI\n', D['control'], 1),
    ('two reasons on one line', b'@r\nA\x01\xc3\n+\nIII\n', D['high_byte'], 1),
    ('a byte that fills a line behind the last record', OK + b'\n \x02\n', D['title'], 4),        # (no blank, no tab: the line counts)
]


def random_fastq(rng, n, crlf=False, at_quality=False, dup=False, empties=False):
    """n records like tests/test_fastq.py's files (no blank lines between records: those are the host reader's)."""
    nl = '\r\n' if crlf else '\n'
    out = []
    for i in range(n):
        length = 0 if (empties and i % 5 == 2) or i % 97 == 5 else int(rng.integers(1, 400))
        name = 'read%d' % (i // 2 if dup else i)
        title = '@%s_Basecall_2D_template:extra ch=%d' % (name, i) if i % 3 else '@%s:x runid=7' % name
        seq = ''.join('ACGT'[c] for c in rng.integers(0, 4, length))
        qual = ''.join(chr(33 + int(q)) for q in rng.integers(0, 60, length))
        if at_quality and length:
            qual = '@' + qual[1:]                             # phred 31: a quality line that looks like a title
        out.append(title + nl + seq + nl + '+' + nl + qual + nl)
    return ''.join(out).encode('ascii')


KINDS = {'plain': {}, 'crlf': dict(crlf=True), 'at_quality': dict(at_quality=True), 'dup': dict(dup=True), 'empties': dict(empties=True)}


def statement(text):
    """read_qual.extract_read_quality_py on the bytes -> its dict."""
    fd, path = tempfile.mkstemp(suffix='.fastq')
    try:
        with os.fdopen(fd, 'wb') as f:
            f.write(text)
        return extract_read_quality_py(path)
    finally:
        os.remove(path)


def same_value(x, y):
    return type(x) is np.float64 and type(y) is np.float64 and ((math.isnan(x) and math.isnan(y)) or x == y)


def assert_same_dict(got, want, what=''):
    assert list(got.keys()) == list(want.keys()), what
    for key in got:
        assert same_value(got[key], want[key]), (what, key, got[key], want[key])


def assert_pairs(keys, means, pairs, what=''):
    assert isinstance(means, np.ndarray) and means.dtype == np.float64
    assert keys == [k for k, _ in pairs], what
    for got, (_, want) in zip(means, pairs):
        assert same_value(got, np.float64(want)), (what, got, want)
