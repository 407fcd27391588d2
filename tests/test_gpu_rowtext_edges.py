"""Rows written on the GPU (mc_rowtext.hip) at the numbers' edges, end to end: read qualities at the ends of the row writer's range
and past them, slot means that are rounding residues (exponent form, below 1e-3: the 128-bit digit generation), another base's
labels.  The streamed file must be the one-table path's byte for byte, and the shards must come from the device or the host formatter
as the numbers they hold say."""
import contextlib
import io
import math
import os
import random

import numpy as np
import pytest

from tests.test_gpu_rowtext import COMP, MODEL, write_case

pytestmark = pytest.mark.gpu

MODEL_GENERAL = os.path.join(os.path.dirname(MODEL), 'r94_model_NN_6_m6A.npz')       # one sub-model ('general'): any base


def run_extract(paths, qual, env, qual_thresh=-1e300, model=MODEL, base='A', motif='A'):
    """extract_features on the whole file with read qualities `qual` -> (the .diffs text, shards whose rows the device wrote, shards)."""
    from mcaller_amd import extract_contexts as ec
    keys = ('MCALLER_NO_STREAM', 'MCALLER_STREAM_SHARDS', 'MCALLER_DEVICE_ROWS', 'MCALLER_ROW_TEXT_ROOM', 'MCALLER_HOST_PARSER')
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    tmp = paths['tsv'][:-4] + '.diffs.6.tmp0'
    ec.stream_features.last_clock = None
    try:
        if os.path.exists(tmp):
            os.remove(tmp)
        with contextlib.redirect_stdout(io.StringIO()):
            ec.extract_features(paths['tsv'], paths['fasta'], qual, 6, 0, qual_thresh, model, 'NN', 0, endline=os.path.getsize(paths['tsv']),
                                train=False, base=base, motif=motif)
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    clock = ec.stream_features.last_clock or {}
    return open(tmp, 'rb').read(), clock.get('device_rows', 0), clock.get('shards', 0)


def reads_in_file_order(path):
    seen = {}
    with open(path) as f:
        next(f)
        for line in f:
            seen.setdefault(line.split('\t', 4)[3], None)
    return list(seen)


def streamed_equals_one_table(paths, qual, **kw):
    want, _, _ = run_extract(paths, qual, {'MCALLER_NO_STREAM': '1'}, **kw)
    got, n_dev, n = run_extract(paths, qual, {'MCALLER_STREAM_SHARDS': '5'}, **kw)
    assert want.count(b'\n') > 200
    assert got == want
    assert n >= 3
    return want, n_dev, n


def quality_column(text):
    return [line.split(b'\t')[4].rsplit(b',', 1)[1] for line in text.splitlines()]


EDGE_QUALITIES = [1e-29, math.ldexp(1.0, -90), 1e-5, 0.1 + 0.2, 1 / 3, 123456789.125, 999999999.9999999, 7.055265349382997,
                  0.30000000000000004, 2.9802322387695312e-08, 1.850371707708594e-17, 12345678.901234567, 100000000.0, 1e8 + 0.5,
                  -2.5, -1e-29, -999999999.9999999, -0.0, 0.0, 9.999999999999999e-05, 1e-4, 5.551115123125783e-17]


def test_edge_qualities_on_reads_with_records_are_printed_on_the_device(tmp_path):
    paths, _ = write_case(str(tmp_path), 41, edge_reads=False, decimals=(2,))
    names = reads_in_file_order(paths['tsv'])
    qual = {name: EDGE_QUALITIES[i % len(EDGE_QUALITIES)] for i, name in enumerate(names)}
    want, n_dev, n = streamed_equals_one_table(paths, qual)
    assert n_dev == n
    printed = set(quality_column(want))
    assert {b'1e-29', b'999999999.9999999', b'-2.5', b'8.077935669463161e-28', b'12345678.901234567', b'100000000.0'} <= printed, printed


def test_out_of_range_qualities_on_reads_with_records_go_to_the_host(tmp_path):
    """The first reads of the file have qualities the row writer refuses: the shards that hold them come from the host formatter,
    the others from the device."""
    paths, _ = write_case(str(tmp_path), 43, edge_reads=False, decimals=(2,))
    names = reads_in_file_order(paths['tsv'])
    rng = random.Random(43)
    qual = {name: round(rng.uniform(3, 40), 12) for name in names}
    bad = [float(np.nextafter(1e-29, 0.0)), 1e9, 5e-324, float('nan'), float('inf'), -1e9]
    for name, q in zip(names[:len(bad)], bad):
        qual[name] = q
    want, n_dev, n = streamed_equals_one_table(paths, qual)
    assert 0 < n_dev < n
    printed = set(quality_column(want))
    assert len({b'9.999999999999998e-30', b'1000000000.0', b'5e-324', b'nan', b'inf', b'-1000000000.0'} & printed) >= 3, printed


def write_residue_case(d, seed, n_reads=30, sparse_every=0):
    """Reads on one contig whose positions have 2 to 5 events, their (event - model) differences chosen so that the slot's sum
    cancels exactly (0.1, 0.2, -0.3) or leaves a tiny mean (0.0001, 0, 0): the means are rounding residues like 1.850371707708594e-17
    and small numbers like 3.3333333333333335e-05.  sparse_every: every such read has an event at every other position only (each
    of its windows has an empty slot: no row at skip threshold 0)."""
    rng = random.Random(seed)
    L = 6000
    seq = ''.join(rng.choice('ACGT') for _ in range(L))
    paths = dict(tsv=os.path.join(d, 'res.eventalign.tsv'), fasta=os.path.join(d, 'ref.fasta'), fastq=os.path.join(d, 'reads.fastq'))
    with open(paths['fasta'], 'w') as fa:
        fa.write('>chr_r\n' + '\n'.join(seq[i:i + 60] for i in range(0, L, 60)) + '\n')
    patterns = [(0.1, 0.2, -0.3), (0.0001, 0.0, 0.0), (0.2, -0.3, 0.1), (0.7, 0.1, -0.8), (1.1, 2.2, -3.3), (0.0001, 0.0),
                (0.0002, 0.0, 0.0, 0.0, 0.0), (0.1, 0.2, -0.3, 0.0), (0.3, -0.1, -0.2, 0.0001, 0.0), (0.0003, 0.0, 0.0)]
    model = {}
    names = []
    with open(paths['tsv'], 'w') as out, open(paths['fastq'], 'w') as fq:
        out.write('contig\tposition\treference_kmer\tread_index\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\t'
                  'model_kmer\tmodel_mean\tmodel_stdv\tstandardized_level\n')
        for i in range(n_reads):
            length = rng.randint(200, 700)
            s = rng.randint(10, L - 16 - length)
            rev = rng.random() < 0.5
            read = 'res-%04d-%08x' % (i, rng.getrandbits(32))
            names.append(read)
            fq.write('@%s\nACGTACGTACGT\n+\n%s\n' % (read, ''.join(chr(33 + rng.randint(3, 40)) for _ in range(12))))
            sparse = sparse_every and i % sparse_every == sparse_every - 1
            positions = list(range(s, s + length, 2 if sparse else 1))
            pats = [rng.choice(patterns) if rng.random() < 0.7 else tuple(rng.randrange(-300, 300) / 100 for _ in range(rng.randint(1, 3)))
                    for _ in positions]
            if rev:
                pats = [tuple(reversed(p)) for p in pats]
            total = sum(len(p) for p in pats)
            idx = 1000 + (total if rev else 0)
            for p, deltas in zip(positions, pats):
                ref_kmer = seq[p:p + 6]
                mk = ref_kmer if not rev else ''.join(COMP[c] for c in reversed(ref_kmer))
                mu = model.setdefault(mk, round(rng.uniform(55.0, 117.0), 2))
                for dl in deltas:
                    out.write('%s\t%d\t%s\t%s\tt\t%d\t%.4f\t1.500\t0.00200\t%s\t%.2f\t1.50\t0.10\n' % (
                        'chr_r', p, ref_kmer, read, idx, mu + dl, mk, mu))
                    idx += -1 if rev else 1
    return paths, names


def test_residue_slot_means_are_printed_on_the_device(tmp_path):
    paths, names = write_residue_case(str(tmp_path), 47)
    rng = random.Random(47)
    qual = {name: round(rng.uniform(3, 40), 10) for name in names}
    want, n_dev, n = streamed_equals_one_table(paths, qual)
    assert n_dev == n
    means = [m for line in want.splitlines() for m in line.split(b'\t')[4].split(b',')[:-1]]
    assert any(b'e-' in m for m in means), 'no slot mean in exponent form'
    assert any(m not in (b'0', b'0.0', b'-0.0') and 0.0 < abs(float(m)) < 1e-3 for m in means), 'no slot mean below 1e-3'
    assert b'1.850371707708594e-17' in want or b'-1.850371707708594e-17' in want or b'1.3877787807814457e-17' in want


def test_out_of_range_qualities_on_reads_without_rows_leave_every_shard_on_the_device(tmp_path):
    """k_rt_digits makes digits for every read's quality, printable or not; whether a row needs them is the row's business: reads
    whose every window has an empty slot write no row, so their nan / inf / 1e9 qualities send no shard to the host."""
    paths, names = write_residue_case(str(tmp_path), 53, n_reads=36, sparse_every=3)
    rng = random.Random(53)
    qual = {name: round(rng.uniform(3, 40), 10) for name in names}
    bad = [float('nan'), float('inf'), 1e9, 5e-324, float(np.nextafter(1e-29, 0.0)), 1e300]
    sparse = [name for i, name in enumerate(names) if i % 3 == 2]
    for j, name in enumerate(sparse):
        qual[name] = bad[j % len(bad)]
    want, n_dev, n = streamed_equals_one_table(paths, qual)
    assert n_dev == n
    for name in sparse:
        assert name.encode() not in want


def test_another_base_and_its_labels(tmp_path):
    """-b C with a C motif: labels 'mC' / 'C' instead of 'm6A' / 'A' (a one-sub-model classifier: any next base), edge qualities."""
    paths, _ = write_case(str(tmp_path), 59, edge_reads=False, decimals=(2, 4))
    names = reads_in_file_order(paths['tsv'])
    qual = {name: EDGE_QUALITIES[(3 * i) % len(EDGE_QUALITIES)] for i, name in enumerate(names)}
    want, n_dev, n = streamed_equals_one_table(paths, qual, model=MODEL_GENERAL, base='C', motif='C')
    assert n_dev == n
    labels = {line.split(b'\t')[6] for line in want.splitlines()}
    assert labels == {b'mC', b'C'} or labels in ({b'mC'}, {b'C'}), labels
