"""mc_decimal.h, the host build (mc_parse_double): every string it accepts is Python's float() bit for bit, what it does not accept
it declines, and nothing inside its stated range is declined (tests/decimal_cases.py builds the strings)."""
import pytest

from tests import decimal_cases as D


def parse(s):
    from mcaller_amd import _lib
    return _lib.parse_double(s.encode('latin-1'))


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_accepted_strings_are_float_bit_for_bit(name):
    strings = getattr(D, 'set_' + name)()
    wrong, declined_inside, accepted_outside = [], [], []
    for s in strings:
        got = parse(s)
        if got is None:
            if D.in_range(s):
                declined_inside.append(s)
        else:
            if not D.in_range(s):
                accepted_outside.append(s)
            if D.bits(got) != D.bits(float(s)):
                wrong.append((s, got, float(s)))
    assert not wrong, wrong[:5]
    assert not declined_inside, declined_inside[:5]
    assert not accepted_outside, accepted_outside[:5]
    if name == 'a':                                           # repr() of such a double: at most 17 digits, exponent >= -23 -- all inside
        assert all(D.in_range(s) for s in strings)


def test_zero_keeps_its_sign():
    assert D.bits(parse('-0.0')) == D.bits(-0.0) != D.bits(parse('0.0'))
    assert D.bits(parse('-0e99')) == D.bits(-0.0)


def test_declines():
    accepted = [s for s in D.set_e() if parse(s) is not None]
    assert not accepted, accepted
