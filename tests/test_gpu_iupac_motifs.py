"""--motifs on the GPU: the site masks of a set of degenerate motifs made on the device (mc_ctx_set_reference_iupac: k_ref_planes,
k_mark_iupac) against the host's marking; the records of the passes that read such masks against the oracle; the command line
file to file against `-p` fed the brute force's site list (tests/iupac_sites.py), against `-m` and against make_bed."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest

from tests import helpers as H
from tests import iupac_cases as IC
from tests import iupac_sites as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from mcaller_amd.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope='module')
def td(tmp_path_factory):
    return H.testdata_paths(str(tmp_path_factory.mktemp('testdata')))


@pytest.mark.parametrize('spec,base', IC.SPECS)
def test_masks_from_the_device_equal_the_hosts_marking(dev, tmp_path, spec, base):
    """Bases, both strand masks and the site numbering, checked as tests/test_gpu_refmark.py checks them."""
    from mcaller_amd import refmark
    contigs = IC.contigs_for(spec, base)
    fa = str(tmp_path / 'r.fa')
    IC.write_fasta(fa, contigs)
    ref = refmark.MarkedReference(fa, base, refmark.parse_motifs(spec, base), None)
    assert ref.motif_for_the_device() is None
    raw = ref.raw_arrays()
    dev.set_reference_iupac(raw, ref.iupac_for_the_device())
    n_contigs = len(ref.records)
    seq, mf, mr, rf, rr, site_base, n_sites = dev.fetch_reference(int(raw['n_seq_bytes']), int(raw['n_words']), n_contigs)
    for cid in range(n_contigs):
        ref.mark(cid)
    want = ref.device_arrays()                      # every contig marked (mc_mark_iupac): the same layout
    assert np.array_equal(raw['contig_len'], want['contig_len']) and np.array_equal(raw['word_off'], want['word_off'])
    assert np.array_equal(raw['seq_off'], want['seq_off'])
    assert np.array_equal(seq, want['seq'][:len(seq)]), spec
    for got, name in ((mf, 'mbits_fwd'), (mr, 'mbits_rev')):
        if not np.array_equal(got, want[name]):
            w = int(np.nonzero(got != want[name])[0][0])
            cid = int(np.searchsorted(want['word_off'], w, side='right')) - 1
            raise AssertionError('%s: %s differs first at word %d (contig %s, word %d): %08x vs %08x' % (
                spec, name, w, contigs[cid][0], w - int(want['word_off'][cid]), int(got[w]), int(want[name][w])))
    run, k = 0, 0
    for cid in range(n_contigs):
        w0 = int(want['word_off'][cid])
        w1 = int(want['word_off'][cid + 1]) if cid + 1 < n_contigs else len(want['mbits_fwd'])
        for bits, rank in ((want['mbits_fwd'], rf), (want['mbits_rev'], rr)):
            pc = np.array([bin(int(x)).count('1') for x in bits[w0:w1]], dtype=np.int64)
            assert np.array_equal(rank[w0:w1], np.concatenate([[0], np.cumsum(pc)[:-1]])), (spec, cid)
            assert site_base[k] == run
            run += int(pc.sum())
            k += 1
    assert n_sites == run and run > 100
    # ... and the host's marking is the brute force's (every planted occurrence included)
    for cid, (name, s) in enumerate(contigs):
        assert tuple(ref.meth[cid]) == S.strings(s, spec, base), (spec, name)


def test_the_library_refuses_a_layout_its_kernels_would_index_past(dev, tmp_path):
    from mcaller_amd import refmark
    from mcaller_amd._lib import McError
    fa = str(tmp_path / 'r.fa')
    IC.write_fasta(fa, [('a', 'GATC' * 20), ('b', 'GACTC' * 9)])
    ref = refmark.MarkedReference(fa, 'A', refmark.parse_motifs('GANTC', 'A'), None)
    spec = ref.iupac_for_the_device()
    for key, value in (('contig_len', [80, 4000]), ('seq_off', [0, 4000]), ('word_off', [0, 3]), ('word_off', [0, 50])):
        raw = ref.raw_arrays()
        raw[key] = np.array(value, dtype=np.int64)
        with pytest.raises(McError):
            dev.set_reference_iupac(raw, spec)


# Site densities of about 1/128, 1/32 and 1/4 of the bases (both strands counted) on random sequence: 4^-4, 4^-2 / 4, 4^-1 / 2 per strand
DENSITY_SPECS = ('GANTC', 'GAYR', 'AR')


def _micro_case():
    for case in H.micro_cases():
        a = case['args']
        if case['flavour'] == 'dense' and not a['train'] and a['base'] == 'A' and a['k'] == 6 and case['positions'] is None:
            return case
    raise AssertionError('no dense micro-case')


def test_records_from_iupac_masks_equal_the_oracle(dev, td, tmp_path):
    """A micro-case table and the testdata: HIP records == the oracle's with the host's mask arrays; the cases lie on both sides
    of the scan's switch (n_sites * 64 > total length: the dense scan)."""
    from mcaller_amd import extract_contexts as ec
    from mcaller_amd import refmark
    from mcaller_amd.read_qual import extract_read_quality
    case = _micro_case()
    (tmp_path / 'micro').mkdir()
    micro = H.materialise(case, str(tmp_path / 'micro'))
    dense, n_records = [], 0
    for paths, model in ((micro, case['args']['model']), (td, 'r95')):
        r2q = extract_read_quality(paths['fastq'])
        for spec in DENSITY_SPECS:
            with contextlib.redirect_stdout(io.StringIO()):
                P = ec.prepare(paths['tsv'], paths['fasta'], r2q, 0, os.path.getsize(paths['tsv']), 'A', refmark.parse_motifs(spec, 'A'), None)
            arrays = P.ref.device_arrays()
            n_sites = sum(bin(int(x)).count('1') for x in arrays['mbits_fwd']) + sum(bin(int(x)).count('1') for x in arrays['mbits_rev'])
            dense.append(n_sites * 64 > int(arrays['contig_len'].sum()))
            modelset = H.load_modelset(model)
            rec = ec.compute(P, 6, 0, 0.0, modelset, 'A', False, device=dev)
            orc = H.oracle_records(P.table, arrays, P.qual, 6, 0, 0.0)
            _, weights, _, soc = ec.submodel_setup(modelset, 'A')
            H.oracle_score(orc, P.table, P.qual, weights, soc, 6)
            H.assert_records_equal(rec, orc, 6)
            n_records += rec.n
    assert True in dense and False in dense, dense
    assert n_records > 0


def run_cli(paths, d, extra, env=None):
    """mCaller on a copy of the eventalign file in directory d -> (the .diffs.6 path, shards the stream cut it into)."""
    from mcaller_amd import mCaller, extract_contexts as ec
    os.makedirs(d)
    tsv = os.path.join(d, os.path.basename(paths['tsv']))
    shutil.copy(paths['tsv'], tsv)
    model = os.path.join(H.MODELS, 'r95_twobase_model_NN_6_m6A.npz')
    keys = ('MCALLER_NO_STREAM', 'MCALLER_STREAM_SHARDS', 'MCALLER_DEVICE_ROWS')
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env or {})
    ec.stream_features.last_clock = None
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mCaller.main(extra + ['-r', paths['fasta'], '-e', tsv, '-f', paths['fastq'], '-d', model])
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return tsv[:-4] + '.diffs.6', (ec.stream_features.last_clock or {}).get('shards', 0)


def site_list(fasta, spec, base, path):
    """The brute force's sites of every contig as a positions file."""
    from oracle import py_oracle
    with open(path, 'w') as fh:
        for name, seq in py_oracle.read_fasta(fasta):
            for strand, sites in zip('+-', S.strands(seq, spec, base)):
                fh.write(''.join('%s\t%d\t%s\n' % (name, p, strand) for p in np.nonzero(sites)[0]))
    return path


def test_file_to_file_motifs_equal_positions_mode_on_the_site_list(td, tmp_path):
    """`--motifs GANTC,GATC` writes the bytes of `-p <the brute force's sites>`: as the CLI runs it, as one table, and with the host's
    row formatter.  (The testdata is one read; the test below streams several shards for certain.)"""
    spec = 'GANTC,GATC'
    posfile = site_list(td['fasta'], spec, 'A', str(tmp_path / 'sites.txt'))
    want = open(run_cli(td, str(tmp_path / 'p'), ['-p', posfile])[0], 'rb').read()
    assert want.count(b'\n') > 10
    for tag, env in (('streamed', {}), ('one_table', {'MCALLER_NO_STREAM': '1'}), ('host_rows', {'MCALLER_DEVICE_ROWS': '0'})):
        got = open(run_cli(td, str(tmp_path / tag), ['--motifs', spec], env)[0], 'rb').read()
        assert got == want, tag


@pytest.mark.parametrize('spec', ['GANTC,GATC', 'AA', 'NAN,CRAANNNNNNNTGC:3+4'])
def test_streamed_shards_scan_the_masks_the_device_made(tmp_path, monkeypatch, spec):
    """Three contigs, 36 reads, streamed in 3 and in 8 shards: the masks come from mc_ctx_set_reference_iupac, once, before the
    first shard, and the rows are the bytes of `-p <the brute force's sites>` run as one table."""
    from mcaller_amd.device import Device
    from tests import test_gpu_rowtext as RT
    made_on_device = []
    setter = Device.set_reference_iupac
    monkeypatch.setattr(Device, 'set_reference_iupac', lambda self, *a: (made_on_device.append(1), setter(self, *a))[1])
    os.makedirs(str(tmp_path / 'case'))
    paths, _ = RT.write_case(str(tmp_path / 'case'), 21)
    posfile = site_list(paths['fasta'], spec, 'A', str(tmp_path / 'sites.txt'))
    out, _ = run_cli(paths, str(tmp_path / 'p'), ['-p', posfile], {'MCALLER_NO_STREAM': '1'})
    want = open(out, 'rb').read()
    assert want.count(b'\n') > 20 and not made_on_device
    for tag, env in (('s3', {'MCALLER_STREAM_SHARDS': '3'}), ('s8_host_rows', {'MCALLER_STREAM_SHARDS': '8', 'MCALLER_DEVICE_ROWS': '0'})):
        del made_on_device[:]
        out, shards = run_cli(paths, str(tmp_path / tag), ['--motifs', spec], env)
        assert open(out, 'rb').read() == want, tag
        assert shards >= 2 and made_on_device == [1], (tag, shards, made_on_device)


def test_file_to_file_motifs_gatc_is_dash_m_gatc(td, tmp_path):
    got = open(run_cli(td, str(tmp_path / 'm'), ['--motifs', 'GATC'])[0], 'rb').read()
    assert got == open(os.path.join(H.GOLDEN, 'ref_outputs', 'motif_GATC.diffs.6'), 'rb').read()


def test_file_to_file_motifs_with_bed_equals_make_bed_over_the_rows(td, tmp_path):
    from mcaller_amd import make_bed
    d = str(tmp_path / 'bed')
    out, _ = run_cli(td, d, ['--motifs', 'GANTC,GATC', '--bed', '--bed_min_depth', '1'])
    bed = os.path.join(d, 'masonread1.methylation.summary.bed')
    got = open(bed, 'rb').read()
    os.remove(bed)
    with contextlib.redirect_stdout(io.StringIO()):
        make_bed.main(['-f', out, '-d', '1', '-t', '0.5'])
    assert got == open(bed, 'rb').read() and got.count(b'\n') > 0
