"""The files of tests/bed_files.py have the properties tests/test_gpu_bed.py relies on (no GPU needed): they are in scope of
the device summary, the host function takes every one of them, their keys repeat and differ in single fields."""
import contextlib
import io

import pytest

from tests import bed_files as B

N_RANDOM = 300


def host_bytes(tmp_path, text, opts, name='x.diffs.6'):
    from mcaller_amd import make_bed
    src, dst = tmp_path / name, tmp_path / (name + '.out')
    src.write_bytes(text)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        n = make_bed.summarise_diffs(str(src), str(dst), opts['depth'], opts['thresh'], control=opts['control'],
                                     with_probs=opts['with_probs'], gff=opts['gff'])
    return dst.read_bytes(), buf.getvalue(), n


def in_scope(text, opts):
    """What the device summary takes (include/mcaller_hip.h), restated on the host."""
    if opts['gff'] and opts['with_probs']:
        return False
    if any(b >= 0x7f or (b < 0x20 and b not in (9, 10)) for b in text):
        return False
    lines = text.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    for line in lines:
        f = line.split(b'\t')
        if len(line) > 65535 or len(f) not in (7, 8) or not (1 <= len(f[2]) <= 9 and f[2].isdigit()) or not f[3] or not f[6]:
            return False
        if len(f) == 7 and opts['with_probs']:
            return False
    return True


def test_make_bed_knows_the_device_flag():
    from mcaller_amd import make_bed
    args = make_bed.build_parser().parse_args(['-f', 'x.diffs.6', '--device'])
    assert args.device is True
    assert make_bed.build_parser().parse_args(['-f', 'x.diffs.6']).device is False
    assert '(mcaller_amd)' in make_bed.build_parser().format_help().split('--device')[-1]


def test_random_files_are_in_scope_and_pass_the_host_function(tmp_path):
    seen_opts, n_rows, multi = set(), [], 0
    for seed in range(N_RANDOM):
        text, opts = B.random_case(seed)
        assert in_scope(text, opts), seed
        out, said, n = host_bytes(tmp_path, text, opts)
        assert out.count(b'\n') == n and ('loci found with min depth %d reads' % opts['depth']) in said
        entries = B.host_entries(text)
        multi += any(e[1] > 1 for e in entries.values())
        n_rows.append(text.count(b'\n') + (not text.endswith(b'\n')))
        seen_opts.add((opts['control'], opts['with_probs'], opts['gff']))
    assert min(n_rows) == 1 and max(n_rows) == 400 and {255, 256, 257} <= set(n_rows)
    assert len(seen_opts) == len(B.option_sets()) == 6
    assert multi > N_RANDOM * 0.7              # keys repeat: most files (all but the smallest) have an entry of several rows


def test_keys_differ_in_every_single_field():
    text, options = B.edge_cases()['single_field_keys']
    keys = list(B.host_entries(text))
    assert len(keys) == 5
    for field in range(4):                     # (chrom, pos, strand, context)
        assert any(sum(a[i] != b[i] for i in range(4)) == 1 and a[field] != b[field] for a in keys for b in keys), field
    assert ('chr1', '123', '+', 'AMA') in keys and ('chr1', '0123', '+', 'AMA') in keys and ('chr11', '123', '+', 'AMA') in keys


def test_edge_files_have_their_shapes(tmp_path):
    cases = B.edge_cases()
    for name, (text, options) in cases.items():
        for opts in options:
            assert in_scope(text, opts), name
    for delta in (-1, 0, 1):
        text, at = B.tile_edge_text(delta)
        assert at == B.TILE + delta and text[at - 1:at] == b'\n' and text[at:at + 5] == b'chr11'
    assert len(cases['text_ends_on_tile'][0]) == B.TILE and cases['text_ends_on_tile'][0].endswith(b'\n')
    assert not cases['no_trailing_newline'][0].endswith(b'\n')
    assert B.host_entries(cases['no_centre_m'][0]) == {}
    hot = B.host_entries(cases['hot_site'][0])
    assert hot[('hot', '42', '-', 'GMTGGMCGTMM')] == [1, 100000] and len(hot) == 51
    deep = B.host_entries(cases['interleaved_vo'][0])
    assert deep[('deep', '9', '+', 'TTMTCMTTCTG')][1] == 5000 and len(deep) == 1001
    wide = cases['interleaved_vo_wide'][0]
    assert B.host_entries(wide)[('deep', '9', '+', 'TTMTCMTTCTG')][1] == 70000 and wide.count(b'\n') > 65536
    lines = cases['long_lines'][0].split(b'\n')
    assert all(sum(len(l) + 1 for l in lines[i:i + 256]) > 48 * 1024 + 16 for i in (0, 256)) and max(map(len, lines)) < 65535
    fr = B.host_entries(cases['fractions'][0])
    assert sorted(tuple(v) for v in fr.values()) == [(0, 4), (1, 3), (1, 7), (2, 3), (4, 4)]
    out, _, n = host_bytes(tmp_path, *[cases['hot_site'][0], cases['hot_site'][1][0]])
    assert n == 51 and b'\t1e-05\t' in out


@pytest.mark.parametrize('name', sorted(B.decline_cases()))
def test_decline_files_are_out_of_scope(name):
    text, opts, reason, line = B.decline_cases()[name]
    assert not in_scope(text, opts)
    assert 1 <= reason <= 8 and 0 <= line <= text.count(b'\n')
