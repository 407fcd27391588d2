"""Decimal strings for mc_decimal.h's host and device builds (tests/test_decimal.py, tests/test_gpu_decimal.py): built once, seeded.

  a  repr(x) of 60 000 finite doubles with 1e-7 <= |x| < 1e9 (log-uniform magnitudes, means of 4-decimal values as a `.train` row
     holds them), and +-0.0
  b  40 000 strings "%de%d": 1-19 digits, exponent -27 .. 27
  c  exact half-way decimals of at most 19 digits -- (2m + 1) * 2^e, m a 53-bit significand, written out with `fractions` -- and
     the same with the last digit one up and one down
  d  shapes of the grammar: sign, bare point, capital E, leading and trailing zeros, zeros with any exponent, "%.4f" forms
  e  what the header declines, never guesses

`in_range(s)` is the range of the header as its issue states it, worked out with `decimal` (not with the code under test): the
significand without leading and trailing zeros has at most 19 digits and the exponent that goes with it is within +-27; zero is
always inside.  A grammatical string outside it (a few of b: "10e27" is 1e28) must be declined, one inside must not be."""
import decimal
import functools
import random
import struct
from fractions import Fraction


def bits(x):
    return struct.pack('<d', x)


def in_range(s):
    sign, digits, exp = decimal.Decimal(s).as_tuple()
    digits = list(digits)
    while digits and digits[0] == 0:
        digits.pop(0)
    if not digits:
        return True
    while digits[-1] == 0:
        digits.pop()
        exp += 1
    return len(digits) <= 19 and -27 <= exp <= 27


@functools.lru_cache(maxsize=None)
def set_a():
    rng = random.Random(20240611)
    out = ['0.0', '-0.0']
    while len(out) < 40002:
        x = rng.choice((-1.0, 1.0)) * 10.0 ** rng.uniform(-7.0, 9.0)
        if 1e-7 <= abs(x) < 1e9:
            out.append(repr(x))
    while len(out) < 60002:                                   # slot means: a sum of 1-6 four-decimal values over their count
        n = rng.randint(1, 6)
        x = sum(rng.randint(-150000, 150000) / 1e4 for _ in range(n)) / n
        if 1e-7 <= abs(x) < 1e9:
            out.append(repr(x))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def set_b():
    rng = random.Random(7)
    out = []
    for i in range(40000):
        nd = 1 + i % 19
        w = rng.randrange(10 ** (nd - 1), 10 ** nd) if nd > 1 else rng.randrange(0, 10)
        out.append('%de%d' % (w, rng.randint(-27, 27)))
    return tuple(out)


def _decimal_of(fr):
    """The exact decimal expansion of a Fraction with a power-of-two denominator -> (digits, k): the value is digits * 10^-k."""
    k = 0
    while fr.denominator != 1:
        fr *= 10
        k += 1
    digits = str(fr.numerator)
    return digits, k


@functools.lru_cache(maxsize=None)
def set_c():
    rng = random.Random(11)
    out = []
    for i in range(3000):
        m = rng.randrange(1 << 52, 1 << 53)
        e = rng.randint(-3, 7)
        digits, k = _decimal_of(Fraction(2 * m + 1) * Fraction(2) ** (e - 1))
        if len(digits) > 19:
            continue
        for delta in (0, 1, -1):
            d = str(int(digits) + delta)
            if len(d) > 19:
                continue
            if i % 2 and 0 < k < len(d):
                out.append(d[:len(d) - k] + '.' + d[len(d) - k:])
            else:
                out.append('%se-%d' % (d, k) if k else d)
    assert len(out) > 3000
    return tuple(out)


@functools.lru_cache(maxsize=None)
def set_d():
    rng = random.Random(13)
    out = ['+1.5', '.5', '5.', '1E5', '007.50', '1.2300e+02', '-0.0', '0.0', '0e99', '0', '-0', '+0.', '.0', '0e-99', '0.000e+999999999999',
           '-.5e-3', '1e0', '1e-0', '1E+05', '1e-05', '100', '1000000000000000000000000000', '0.000000000000000000000000001',
           '1234567890123456789', '9999999999999999999', '12345678901234567890', '1.000000000000000000000000000000', '000000000000000000000001.500000',
           '5e-27', '5e27', '9999999999999999999e27', '9999999999999999999e-27', '1.7976931348623157', '4.9e-7', '2.5', '0.1', '0.3']
    out += ['%.4f' % (rng.randint(-2000000, 2000000) / 1e4) for _ in range(2000)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def set_e():
    return (' 1.5', '1.5 ', '\t1', '1\n', '1_000', '1_0.5', 'inf', '-inf', 'nan', 'infinity', 'Infinity', 'NaN', '+nan',
            '12345678901234567891', '1.2345678901234567891', '0.00012345678901234567891', '1e28', '1e-28', '1e99', '1e-400', '10e27', '0.1e-27',
            '', '.', '+', '-', '+.', 'e5', '.e5', '1e', '1e+', '1e-', '-e1', '0x10', '0x1p3', '0x.8', '1.2.3', '1..2', '--1', '+-1', '1e5.0', '1e1e1',
            '1,5', '1f', 'abc', '1 2', '\x001', '1\x00')


def grammatical():
    """(a) - (d): strings of the grammar; float() parses every one."""
    return set_a() + set_b() + set_c() + set_d()
