"""Part files for the merge behind `-t N` (mCaller.merge_like_sort_uniq and its device path, csrc/merge/mc_rowmerge.hip): a seeded
generator, the edge files and the files the device declines.  A case is a list of parts (bytes), one per part file.  The
yardstick is merge_like_sort_uniq on the same files (host_merge); tests/test_merge_files.py checks that every in-scope case stays
inside what the device is asked to cover."""
import os
import re

import numpy as np

KP_TILE = 16384            # bytes per tile of the line-start kernels (csrc/mc_devparse.inc)
SCATTER_CHUNK = 4096       # items a workgroup of a radix pass scatters (csrc/merge/mc_rowmerge.hip)
SMALL = 32                 # groups up to this size are finished by comparison there

# the names of tests/test_cli_host.py::test_merge_orders_like_sort_n_k2
CLI_HOST_NAMES = ['2289b392-aaaa', 'cc1d-ffff', '0041', '41zz', '-7-neg', '3.5e', '3.25', '10', '9', '  spaced', '2289b392-aaaa',
                  '007', '7', '1e3', '.5', '-.5x', 'abc']
NUMERIC_KEYS = CLI_HOST_NAMES + ['000000000000000007', '7', '-0', '-', 'abc', '', '-7', '-.5x', '.5', '3.', '3.25', '0.50', '0.5', '-0.50',
                                 '-.5', '-3.25', '-3.', '.', '-.', '0', '00', '0.0', '-0.0', '.0', '1e3', '1', '+5', '5+', '--5', '-5-',
                                 '999999999999999999', '-999999999999999999', '999999999999999998', '.999999999999999999',
                                 '-.999999999999999999', '999999999999999999.999999999999999999',
                                 '-999999999999999999.999999999999999999', '0000999999999999999999.9999999999999999990000',
                                 '.000000000000000001', '-.000000000000000001', '.0000000000000000000000', '100000000000000000',
                                 '1.000000000000000001', '12.', '12.x', '12..5', '12.5.5', '1-2', '0x10', '\t7', ' \t 8', '7\t9']


def name_rows(names, seed=3, times=3):
    """Rows as tests/test_cli_host.py makes them: the name in field 2."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, nm in enumerate(list(names) * times):
        rows.append(('chr%d\t%s\t%d\tGATCM\t0.1,0.2\t+\tA\t0.%d\n' % (rng.integers(0, 3), nm, rng.integers(0, 50), i % 10)).encode())
    return rows


def deal(rows, n_parts):
    """The rows dealt round-robin over n_parts part files."""
    return [b''.join(rows[i::n_parts]) for i in range(n_parts)]


def counted_lines(n, seed):
    """n lines, shuffled: about half with a numeric key, the others tied at key 0 and told apart by their bytes; a few repeat."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        v = int(rng.integers(0, max(2, n // 2)))
        if i % 2:
            rows.append(b'c\t%d\tp%d\n' % (v, i % 7))
        else:
            rows.append(b'r%d\tx%d\n' % (v, i % 5))
    return rows


def tie_lines(p, n_lines):
    """n_lines lines of key 0 that share their first p bytes and differ at byte p; one of them ends there."""
    prefix = (b'abcdefghijklmnopqrstuvwxyz' * 8)[:p]
    tails = [bytes([c]) for c in (0, 1, 9, 11, 31, 32, 48, 65, 127, 128, 200, 255)] + [b'%c%c' % (66, c) for c in range(60, 60 + n_lines)]
    return [prefix + b'\n'] + [prefix + t + b'\n' for t in tails[:n_lines - 1]]


def one_read(n_rows, seed):
    """One read's rows: they differ only in the position text ('100' sorts before '99')."""
    rng = np.random.default_rng(seed)
    pos = rng.permutation(n_rows) + 90
    return [b'contig_1\t2289b392-1f0a-4c5e-9d3b-aaaaaaaaaaaa\t%d\tGATCAMGATCA\t1.25,-0.5,3.0,0.125,2.5,-1.0\t+\tm6A\t0.75\n' % q for q in pos]


def many_reads(n_reads, seed):
    """Reads of 1-3 rows each, names that start with digits or letters."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_reads):
        name = '%08x-%04x' % (int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 16)))
        for _ in range(int(rng.integers(1, 4))):
            rows.append(('chr1\t%s\t%d\tGATCM\t0.5\t-\tA\t0.25\n' % (name, int(rng.integers(0, 2000)))).encode())
    return rows


def tile_edge_text(start_at, end_on_boundary=False):
    """A text whose marked line starts at byte `start_at`; filler lines of key 0 before it."""
    out, at, i = [], 0, 0
    while start_at - at >= 18:                 # nine-byte lines, then one that fills what is left (9-17 bytes)
        out.append(b'f%04d\tzz\n' % i)
        at += 9
        i += 1
    if start_at > at:
        out.append(b'g' * (start_at - at - 1) + b'\n')
    out.append(b'MARK\t5\there\n')
    text = b''.join(out)
    if end_on_boundary:
        pad = (-len(text)) % KP_TILE
        text += b'e' * (pad - 1) + b'\n' if pad else b''
        assert len(text) % KP_TILE == 0
    return text


def random_file(seed):
    """1-400 lines over small alphabets: contigs, names and positions repeat and differ in single bytes."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 401))
    contigs = [b'c', b'c1', b'c2', b'chr\xe9', b'chrz', b'']
    names = [b'12', b'12a', b'012', b'12.0', b'12.5', b'-3', b'ab', b'abc', b'b', b'', b'7', b'07', b'1e3', b'.5', b'0.50', b'-']
    seps = [b'\t', b' ', b'\t\t', b' \t']
    rows = []
    for _ in range(n):
        kind = int(rng.integers(0, 12))
        if kind == 0:
            rows.append(b'\n')
        elif kind == 1:
            rows.append(contigs[int(rng.integers(0, len(contigs)))] + b'\n')
        else:
            tail = b''.join([b'\t', b'1', b'2', b'a', b'\x00', b'\xff', b' '][int(c)] for c in rng.integers(0, 7, int(rng.integers(0, 12))))
            rows.append(contigs[int(rng.integers(0, len(contigs)))] + seps[int(rng.integers(0, 4))] +
                        names[int(rng.integers(0, len(names)))] + (b'\t%d' % int(rng.integers(0, 12))) + tail + b'\n')
    n_parts = int(rng.integers(1, 4))
    return deal(rows, n_parts)


def edge_cases():
    """{name: parts}: everything the device must reproduce."""
    cases = {}
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, SCATTER_CHUNK + 1):
        cases['count_%d' % n] = [b''.join(counted_lines(n, n))]
    cases['count_70000_short'] = [b''.join(counted_lines(70000, 5))]
    for p in (0, 7, 8, 9, 63, 64, 65, 100):
        cases['tie_at_%d_few' % p] = [b''.join(reversed(tie_lines(p, 5)))]
        cases['tie_at_%d_many' % p] = [b''.join(reversed(tie_lines(p, SMALL + 9)))]
    long_prefix = b'q' * 4000
    cases['two_equal_for_4000'] = [long_prefix + b'y\n' + long_prefix + b'x\n']
    cases['many_equal_for_600'] = [b''.join(b'w' * 600 + b'%02d\n' % (97 - i) for i in range(SMALL + 8))]
    cases['one_read_5000'] = [b''.join(one_read(5000, 1))]
    cases['reads_300'] = deal(many_reads(300, 2), 2)
    cases['newline_before_tab'] = [b'a\n' + b'a\tb\n']
    cases['unsigned_bytes'] = [b'chrz\tx\t1\n' + b'chr\xe9\tx\t1\n' + b'chr\x7f\tx\t1\n' + b'chr\x01\tx\t1\n']
    cases['lone_newline'] = [b'b\t1\n' + b'\n' + b'a\t1\n' + b'\n']
    cases['one_field'] = [b'zzz\n' + b'abc\n' + b'abc\t0\n']
    rows = name_rows(CLI_HOST_NAMES)
    cases['dup_three_apart'] = [rows[0] + rows[1] + rows[0] + rows[2] + rows[3] + rows[0]]
    cases['all_equal_few'] = [rows[0] * 7]
    cases['all_equal_many'] = [rows[0] * (SMALL + 30)]
    cases['dup_in_two_files'] = [rows[0] + rows[1], rows[2] + rows[0]]
    cases['empty_part_between'] = [rows[0], b'', rows[1]]
    cases['cli_host_dealt'] = deal(rows + rows[:7], 3)
    cases['numeric_keys'] = deal(name_rows(NUMERIC_KEYS, seed=4, times=2), 2)
    cases['tile_start_before'] = [tile_edge_text(KP_TILE - 1)]
    cases['tile_start_on'] = [tile_edge_text(KP_TILE)]
    cases['tile_start_after'] = [tile_edge_text(KP_TILE + 1)]
    cases['tile_text_ends_on'] = [tile_edge_text(KP_TILE - 30, end_on_boundary=True)]
    return cases


def decline_cases():
    """{name: (parts, reason name as in _lib.MERGE_DECLINE, 0-based line over all parts)}"""
    rows = name_rows(CLI_HOST_NAMES)
    return {
        'carriage_return': ([rows[0] + rows[1] + b'chr1\tab\r\t3\n' + rows[2]], 'cr', 2),
        'no_final_newline': ([rows[0] + rows[1][:-1], rows[2] + rows[3]], 'no_newline', 1),
        'key_19_digits': ([rows[0] + b'chr1\t1234567890123456789\t3\n' + rows[2]], 'key', 1),
        'fraction_19_digits': ([b'chr1\t0.1234567890123456789\t3\n' + rows[2]], 'key', 0),
        'line_70000_bytes': ([rows[0] + rows[1] + rows[2] + b'L' * 69999 + b'\n' + rows[3]], 'long_line', 3),
    }


_KEY = re.compile(rb'^[^ \t]*[ \t]*-?0*([0-9]*)(?:\.([0-9]+))?')


def key_digits(line):
    """(significant integer digits, fraction digits without trailing zeros) of the line's numeric prefix."""
    m = _KEY.match(line)
    return len(m.group(1)), len((m.group(2) or b'').rstrip(b'0'))


def write_parts(parts, directory, stem='rows'):
    paths = []
    for i, part in enumerate(parts):
        paths.append(os.path.join(str(directory), '%s.tmp%d' % (stem, i)))
        with open(paths[-1], 'wb') as fh:
            fh.write(part)
    return paths


def host_merge(parts, directory):
    """The yardstick: merge_like_sort_uniq over the parts, written as files."""
    from mcaller_amd.mCaller import merge_like_sort_uniq
    paths = write_parts(parts, directory, stem='yardstick')
    out = os.path.join(str(directory), 'yardstick.merged')
    merge_like_sort_uniq(paths, out)
    with open(out, 'rb') as fh:
        blob = fh.read()
    os.remove(out)
    return blob
