"""compare_genomes through a Mauve alignment on the GPU (mcaller_amd/csrc/compare/mc_xmfamap.inc; Device.xmfa_map,
Device.bed_compare(contigs1=, contigs2=), compare_genomes.compare_by_position_device(xmfa_path=)) against the host statement: the
same map and the same bytes on seeded random alignments and on hand-made edges (word, line, contig and workgroup edges, with
poisoned allocations, each with both strands flipped), through small pinned stages, with sixteen hash values; every new decline with
its reason and line and the host's output or error behind it; two alignments on one context."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mcaller_amd import _lib
from mcaller_amd import compare_genomes as CG
from tests import helpers as H
from tests import xmfa_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import get_device
    return get_device()


def lift_of(P, c):
    return dict(xmfa_path=P['xmfa'], fai1=P['fai1'], fai2=P['fai2'], seqs=c['seqs'])


def test_random_alignments(dev, tmp_path):
    paired = 0
    for i, c in enumerate(X.random_cases(40)):
        xs, cs = X.device_makes_it(dev, tmp_path, c, 'r%d.' % i)
        paired += xs['n_paired_blocks']
        assert cs['n_sites'] >= 1
    assert paired >= 40


def test_hand_made_edges_with_poisoned_allocations(tmp_path):
    env = dict(os.environ, MCALLER_POISON='1', PYTHONPATH=H.REPO)
    done = subprocess.run([sys.executable, os.path.join(H.REPO, 'tests', '_xmfa_edges_worker.py'), str(tmp_path)], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0 and b'edges ok' in done.stdout, done.stdout.decode('utf-8', 'replace')[-3000:]


def test_the_alignment_through_small_stages(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('MCALLER_TEXT_STAGE_BYTES', '256')
    c = X.edge_case('line widths')
    assert len(c['xmfa']) > 6 * 256                                    # each of the two stages is written again and again
    xs, _ = X.device_makes_it(dev, tmp_path, c)
    assert xs['n_columns'] == 650 and xs['n_mapped'] == 650


def test_sixteen_hash_values(dev, tmp_path, monkeypatch):
    """No tag tells two keys apart: the comparison of the synthesised key's pieces against the slot's line decides."""
    monkeypatch.setenv('MCALLER_CMP_HASH_MASK', 'f')
    for name in ('block sizes', 'contig edges'):
        _, cs = X.device_makes_it(dev, tmp_path, X.edge_case(name))
        assert cs['n_sites'] >= 6 and cs['longest_probe'] >= 2


BAD = X.bad_xmfas()


@pytest.mark.parametrize('name', sorted(BAD))
def test_every_alignment_the_definition_refuses(dev, tmp_path, name):
    text, reason, line = BAD[name]
    g2, flip, why = dev.xmfa_map(text=text, n1=8, n2=8)
    st = dev.xmfa_map_last_stats()
    print(name, why, st)
    assert g2 is None and flip is None and '(line %d)' % (line + 1) in why
    assert (st['decline_reason'], st['decline_line']) == (_lib.CMP_DECLINE[reason], line)
    with pytest.raises(_lib.McError, match='no alignment map'):           # no map is kept
        dev.bed_compare(text1=b'', text2=b'', contigs1=(['a'], [8], [0, 8]), contigs2=(['b'], [8], [0, 8]))
    c = X.identity_case()
    P = X.write(tmp_path, dict(c, xmfa=text, fai1='a\t8\n', fai2='b\t8\n'))
    with pytest.raises(ValueError, match=r'^xmfa line %d: ' % (line + 1)):
        CG.compare_by_position_device(P['bed1'], P['bed2'], out=str(tmp_path / 'out.tsv'), **lift_of(P, c))


def test_a_genome_too_long_for_the_map(dev):
    g2, flip, why = dev.xmfa_map(text=b'', n1=(1 << 31) - 1, n2=8)
    st = dev.xmfa_map_last_stats()
    assert g2 is None and '2^31' in why and (st['decline_reason'], st['decline_line']) == (_lib.CMP_DECLINE['xmfa_genome'], -1)
    g2, flip, why = dev.xmfa_map(text=b'', n1=8, n2=(1 << 31) - 1)
    assert g2 is None and dev.xmfa_map_last_stats()['decline_reason'] == _lib.CMP_DECLINE['xmfa_genome']


def test_a_map_that_does_not_fit(dev, tmp_path, monkeypatch):
    c = X.edge_case('contig edges')
    P = X.write(tmp_path, c)
    want = CG.compare_rows(P['bed1'], P['bed2'], **lift_of(P, c))
    monkeypatch.setenv('MCALLER_CMP_DEVICE_BYTES', '1000')
    g2, flip, why = dev.xmfa_map(path=P['xmfa'], n1=c['n1'], n2=c['n2'])
    st = dev.xmfa_map_last_stats()
    assert g2 is None and 'do not fit' in why and (st['decline_reason'], st['decline_line']) == (_lib.CMP_DECLINE['memory'], -1)
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(P['bed1'], P['bed2'], out=out, **lift_of(P, c)) == want[1]
    assert CG.last_compare['by'] == 'host' and CG.last_compare['reason'] == why and open(out, 'rb').read() == want[0]


@pytest.mark.parametrize('form', ['+7', '007', '1_0', ' 7', 'x'])
def test_a_start_that_is_not_plain_digits(dev, tmp_path, form):
    c = X.identity_case()
    P = X.write(tmp_path, c)
    lines = c['bed1'].decode().splitlines(True)
    first = lines[1].split('\t')
    open(P['bed1'], 'w').write(lines[0] + '\t'.join([first[0], form] + first[2:]) + ''.join(lines[2:]))
    want = CG.compare_rows(P['bed1'], P['bed2'], **lift_of(P, c))
    contigs = CG.read_fai(P['fai1'])
    assert dev.xmfa_map(path=P['xmfa'], n1=c['n1'], n2=c['n2'])[2] is None
    blob, n, why = dev.bed_compare(path1=P['bed1'], path2=P['bed2'], contigs1=contigs, contigs2=contigs)
    st = dev.bed_compare_last_stats()
    assert blob is None and 'plain digits' in why and '(bed1)' in why and '(line 2)' in why
    assert (st['decline_reason'], st['decline_file'], st['decline_line']) == (_lib.CMP_DECLINE['lift_start'], 1, 1)
    assert dev.bed_compare_last_unaligned() is None
    out = str(tmp_path / 'out.tsv')
    assert CG.compare_by_position_device(P['bed1'], P['bed2'], out=out, **lift_of(P, c)) == want[1]
    assert CG.last_compare['by'] == 'host' and CG.last_compare['reason'] == why and open(out, 'rb').read() == want[0]


def test_a_start_of_many_digits_is_past_its_contig(dev, tmp_path):
    c = X.identity_case()
    P = X.write(tmp_path, c)
    first = c['bed1'].decode().splitlines(True)[0].split('\t')
    open(P['bed1'], 'ab').write(('\t'.join([first[0], '123456789012345'] + first[2:]) + '\t'.join([first[0], '4294967296'] + first[2:])).encode())
    X.device_makes_it(dev, tmp_path, dict(c, bed1=open(P['bed1'], 'rb').read()))


def test_two_alignments_on_one_context(dev, tmp_path):
    a, b = X.edge_case('contig edges'), X.random_case(3)
    Pa, Pb = X.write(tmp_path, a, 'a.'), X.write(tmp_path, b, 'b.')
    want_a, want_b = (CG.compare_rows(P['bed1'], P['bed2'], **lift_of(P, c)) for P, c in ((Pa, a), (Pb, b)))
    tables = {k: (CG.read_fai(P['fai1']), CG.read_fai(P['fai2'])) for k, P in (('a', Pa), ('b', Pb))}
    ga = dev.xmfa_map(path=Pa['xmfa'], n1=a['n1'], n2=a['n2'], seqs=a['seqs'])
    gb = dev.xmfa_map(path=Pb['xmfa'], n1=b['n1'], n2=b['n2'], seqs=b['seqs'])
    assert ga[2] is None and gb[2] is None and len(gb[0]) == b['n1'] + 1
    assert np.array_equal(gb[0], CG.xmfa_map(Pb['xmfa'], b['n1'], b['seqs'], b['n2'])[0])
    blob, n, why = dev.bed_compare(path1=Pb['bed1'], path2=Pb['bed2'], contigs1=tables['b'][0], contigs2=tables['b'][1])
    assert why is None and (blob, n) == want_b
    with pytest.raises(_lib.McError, match='totals'):                      # the first alignment's genomes: not this map's
        dev.bed_compare(path1=Pa['bed1'], path2=Pa['bed2'], contigs1=tables['a'][0], contigs2=tables['a'][1])
    blob, n, why = dev.bed_compare(path1=Pb['bed1'], path2=Pb['bed2'])        # the plain comparison does not look at the map
    assert why is None and (blob, n) == CG.compare_rows(Pb['bed1'], Pb['bed2'])
    dev.xmfa_map_release()
    with pytest.raises(_lib.McError, match='no alignment map'):
        dev.bed_compare(path1=Pb['bed1'], path2=Pb['bed2'], contigs1=tables['b'][0], contigs2=tables['b'][1])
    assert dev.xmfa_map(text=a['xmfa'], n1=a['n1'], n2=a['n2'], seqs=a['seqs'], view=False) == (None, None, None)
    blob, n, why = dev.bed_compare(text1=a['bed1'], text2=a['bed2'], contigs1=tables['a'][0], contigs2=tables['a'][1])
    assert why is None and (blob, n) == want_a and dev.bed_compare_last_unaligned() >= 1
    dev.xmfa_map_release()


def test_cli_device(dev, tmp_path, capfd):
    c = X.random_case(5)
    P = X.write(tmp_path, c)
    CG.main(['--bed1', P['bed1'], '--bed2', P['bed2'], '--xmfa', P['xmfa'], '--fai1', P['fai1'], '--fai2', P['fai2'], '--xmfa_seqs',
             '%d,%d' % c['seqs'], '--device'])
    assert capfd.readouterr().out.encode() == X.expected_rows(c)[0]
    assert CG.last_compare['by'] == 'device' and CG.last_compare['n_unaligned'] == X.expected_rows(c)[2]
