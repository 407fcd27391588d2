"""mc_sort_key (the host build of csrc/mc_sortkey.h, the key of the device merge) against mCaller.numeric_key_k2: the order of
the 128-bit keys is Decimal's order, equality included.  No GPU."""
import ctypes as C

import numpy as np

from tests import merge_files as MF


def sort_key(line):
    from mcaller_amd import _lib
    hi, lo = C.c_uint64(), C.c_uint64()
    rc = _lib.lib().mc_sort_key(line, len(line), C.byref(hi), C.byref(lo))
    return rc, (hi.value << 64) | lo.value


def sign(x):
    return (x > 0) - (x < 0)


def check_pairs(lines, pairs):
    from mcaller_amd.mCaller import numeric_key_k2
    want = [numeric_key_k2(l) for l in lines]
    got = []
    for l in lines:
        rc, k = sort_key(l)
        assert rc == 0, l
        got.append(k)
    for a, b in pairs:
        assert sign(got[a] - got[b]) == sign(want[a].compare(want[b])), (lines[a], lines[b])


def test_the_listed_keys_compare_like_decimal():
    lines = [b'chr1\t' + nm.encode() + b'\t12\tGATCM\n' for nm in MF.NUMERIC_KEYS]
    lines += [b'', b'\n', b'x\n', b'x \n', b'x\t\n', b'x\t-\n', b'x 5\n', b' 5\n', b'\t-5.5\n', b'x\t5', b'x\t5.', b'x\t.']
    check_pairs(lines, [(a, b) for a in range(len(lines)) for b in range(len(lines))])
    zero = sort_key(b'c\tabc\n')[1]
    assert zero == 1 << 127
    for nm in (b'-0', b'-', b'abc', b'', b'0.0', b'-.0', b'000'):
        assert sort_key(b'c\t' + nm + b'\n')[1] == zero
    assert sort_key(b'c\t007\n') == sort_key(b'c\t7\n') and sort_key(b'c\t0.50\n') == sort_key(b'c\t.5\n')
    assert sort_key(b'c\t1e3\n') == sort_key(b'c\t1\n')


def test_random_field_2_strings_compare_like_decimal():
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b'0123456789.-ea \t', dtype=np.uint8)
    lens = rng.integers(0, 13, 100000)
    chars = alphabet[rng.integers(0, len(alphabet), int(lens.sum()))].tobytes()
    lines, at = [], 0
    for n in lens:
        lines.append(b'c\t' + chars[at:at + n] + b'\n')
        at += int(n)
    pairs = list(zip(rng.integers(0, len(lines), 200000).tolist(), rng.integers(0, len(lines), 200000).tolist()))
    # (near pairs too: sorted by the yardstick, neighbours are equal or next to each other)
    from mcaller_amd.mCaller import numeric_key_k2
    order = sorted(range(len(lines)), key=lambda i: numeric_key_k2(lines[i]))
    pairs += list(zip(order[:-1], order[1:]))
    check_pairs(lines, pairs)


def test_the_digit_limits():
    assert sort_key(b'c\t' + b'9' * 18 + b'.' + b'9' * 18 + b'\n')[0] == 0
    assert sort_key(b'c\t' + b'0' * 30 + b'9' * 18 + b'.' + b'9' * 18 + b'0' * 30 + b'\n')[0] == 0
    assert sort_key(b'c\t' + b'1' + b'0' * 18 + b'\n')[0] == 1
    assert sort_key(b'c\t-' + b'1' * 19 + b'\n')[0] == 1
    assert sort_key(b'c\t0.' + b'0' * 18 + b'1\n')[0] == 1
    assert sort_key(b'c\t0.' + b'0' * 18 + b'0\n')[0] == 0
    hi, lo = C.c_uint64(), C.c_uint64()
    from mcaller_amd import _lib
    assert _lib.lib().mc_sort_key(None, 3, C.byref(hi), C.byref(lo)) == -12
