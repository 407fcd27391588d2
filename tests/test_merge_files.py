"""The part files of tests/merge_files.py stay inside what the device merge is asked to cover, so the yardstick alone
(mCaller.merge_like_sort_uniq) never leaves that scope; and the files meant to be declined are outside it.  No GPU."""
import pytest

from tests import merge_files as MF


def in_scope_cases():
    cases = dict(MF.edge_cases())
    for seed in range(300):
        cases['random_%d' % seed] = MF.random_file(seed)
    return cases


def test_every_in_scope_file_ends_in_a_newline_and_holds_no_carriage_return():
    for name, parts in in_scope_cases().items():
        for part in parts:
            assert part == b'' or part.endswith(b'\n'), name
            assert b'\r' not in part, name
            assert max(len(l) for l in part.splitlines(True) or [b'']) <= 65535, name


def test_every_key_is_within_18_and_18_digits():
    seen_max = [0, 0]
    for name, parts in in_scope_cases().items():
        for part in parts:
            for line in part.splitlines(True):
                ni, nf = MF.key_digits(line)
                assert ni <= 18 and nf <= 18, (name, line)
                seen_max = [max(seen_max[0], ni), max(seen_max[1], nf)]
    assert seen_max == [18, 18]                  # the maxima are among the cases


def test_key_digits_reads_the_grammar_of_numeric_key_k2():
    from mcaller_amd.mCaller import numeric_key_k2
    for nm in MF.NUMERIC_KEYS:
        line = b'c\t' + nm.encode() + b'\t1\n'
        ni, nf = MF.key_digits(line)
        _, digits, exp = numeric_key_k2(line).as_tuple()      # (by hand: normalize() rounds to the context's 28 digits)
        digits = list(digits)
        while len(digits) > 1 and digits[-1] == 0 and exp < 0:
            digits.pop()
            exp += 1
        while len(digits) > 1 and digits[0] == 0:
            digits.pop(0)
        if digits == [0]:
            assert (ni, nf) == (0, 0), nm
        else:
            assert nf == max(0, -exp) and ni == max(0, len(digits) + exp), nm


def test_the_edge_files_are_where_they_say():
    cases = MF.edge_cases()
    for name, at in (('tile_start_before', MF.KP_TILE - 1), ('tile_start_on', MF.KP_TILE), ('tile_start_after', MF.KP_TILE + 1)):
        assert cases[name][0].index(b'MARK') == at and cases[name][0][at - 1:at] == b'\n'
    assert len(cases['tile_text_ends_on'][0]) == MF.KP_TILE
    assert cases['count_0'] == [b''] and cases['count_1'][0].count(b'\n') == 1
    assert cases['count_70000_short'][0].count(b'\n') == 70000
    for p in (0, 7, 8, 9, 63, 64, 65, 100):
        lines = cases['tie_at_%d_many' % p][0].splitlines(True)
        assert len(lines) == MF.SMALL + 9 == len(set(lines)) and len({l[:p] for l in lines}) == 1
        assert len({l[:p + 1] for l in lines}) >= 13


@pytest.mark.parametrize('name', sorted(MF.decline_cases()))
def test_the_decline_files_are_out_of_scope(name):
    parts, reason, line = MF.decline_cases()[name]
    whole = b''.join(parts)
    lines = []
    for part in parts:
        lines += part.split(b'\n')[:-1] if part.endswith(b'\n') else part.split(b'\n')
    bad = lines[line]
    if reason == 'cr':
        assert b'\r' in bad and b'\r' not in b'\n'.join(lines[:line])
    elif reason == 'no_newline':
        assert not parts[0].endswith(b'\n') and parts[0].count(b'\n') == line
    elif reason == 'key':
        assert max(MF.key_digits(bad + b'\n')) > 18
    elif reason == 'long_line':
        assert len(bad) + 1 > 65535
    assert whole
