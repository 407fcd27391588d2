"""A `--training_tsv` file read on the GPU (mcaller_amd/csrc/train/mc_trainrows.hip; load_mCaller_data.tsv2matrix_device) gives
tsv2matrix's dicts -- itself pinned to the reference's capture by tests/test_train.py --, key order included and floats bit for
bit; every assertion on values comes with one on WHO made them (load_mCaller_data.last_load): a silent fall-back proves nothing."""
import contextlib
import io
import os
import shutil
import zipfile

import numpy as np
import pytest

from tests import helpers as H
from tests import train_rows_files as T

pytestmark = pytest.mark.gpu

ROWS = os.path.join(H.GOLDEN, 'train', 'training_rows.train')


def both(path):
    """-> (tsv2matrix's dicts, tsv2matrix_device's, last_load)."""
    from mcaller_amd import load_mCaller_data as L
    host = L.tsv2matrix(path, 'A')
    L.last_load = None
    dev = L.tsv2matrix_device(path, 'A')
    return host, dev, L.last_load


def test_the_captured_fixture():
    host, dev, load = both(ROWS)
    assert T.plain(*dev) == T.plain(*host)
    assert load == dict(by='device', reason=None, n_rows=sum(len(v) for v in host[0]['general'].values()))
    for label, rows in dev[0]['general'].items():
        assert isinstance(rows, np.ndarray) and rows.dtype == np.float64 and rows.ndim == 2
        assert dev[1]['general'][label].dtype.kind == 'S' and len(dev[1]['general'][label]) == len(rows)


@pytest.mark.parametrize('n_lines', T.SIZES)
def test_random_files(tmp_path, n_lines):
    from mcaller_amd.device import get_device
    seen = dict(in_place=0, empty_label=0, labels=set(), nf=set())
    for seed in range(6):
        text, info = T.random_file(seed, n_lines)
        path = str(tmp_path / ('s%d.train' % seed))
        open(path, 'wb').write(text)
        host, dev, load = both(path)
        assert load['by'] == 'device' and load['reason'] is None, (seed, load)
        assert T.plain(*dev) == T.plain(*host), seed
        st = get_device().training_rows_last_stats()
        assert st['n_lines'] == n_lines and st['n_labels'] == info['n_labels'] and st['n_kept'] == load['n_rows']
        if n_lines >= 255:                                   # (256 lines and a 40 KB name do not fit the stage; two lines do)
            assert (st['in_place_blocks'] > 0) == (info['long_line'] >= 0), (seed, st)
        # file order, said once more without the host function: the kept rows' contexts of a label, line by line
        by_label = {}
        for line in text.decode('ascii').split('\n'):
            f = line.split('\t')
            if len(f) >= 7:
                feats = f[4].split(',')
                rows = by_label.setdefault(f[6].strip(), [])
                if len(feats) >= 6 and '0' not in feats:
                    rows.append(f[3])
        assert {k: [c.decode('ascii') for c in v.tolist()] for k, v in dev[1]['general'].items()} == by_label
        assert list(dev[1]['general']) == list(by_label)
        seen['in_place'] += st['in_place_blocks'] > 0
        seen['empty_label'] += any(len(v) == 0 for v in dev[0]['general'].values())
        seen['labels'].add(info['n_labels'])
        seen['nf'].add(st['n_features'])
        for label, rows in dev[0]['general'].items():
            assert rows.shape == (len(dev[1]['general'][label]), rows.shape[1])
    if n_lines >= 255:                                       # the generator's variety did reach the device
        assert seen['in_place'] >= 2 and seen['empty_label'] >= 1 and seen['labels'] == {1, 2, 3} and seen['nf'] == {6, 7}


def test_label_table_with_colliding_hashes(tmp_path, monkeypatch):
    """MCALLER_TRAINROWS_HASH_MASK=f leaves 16 hash values and an empty tag: the byte comparison decides which label a row carries."""
    lines = []
    labels = ['L%d' % i for i in range(16)]
    for i in range(600):
        label = labels[(i * 7 + i // 16) % 16]
        lines.append('c\tr\t%d\tAAAAAMGAAAA\t%s\t+\t%s' % (i, ','.join(repr((i * 13 + j) / 8.0 + 0.125) for j in range(6)), label))
    path = str(tmp_path / 'sixteen.train')
    open(path, 'w').write('\n'.join(lines) + '\n')
    monkeypatch.setenv('MCALLER_TRAINROWS_HASH_MASK', 'f')
    host, dev, load = both(path)
    assert load['by'] == 'device' and T.plain(*dev) == T.plain(*host) and len(dev[0]['general']) == 16


GOOD = 'c\tr\t5\tAAAAAMGAAAA\t1.5,2.5,-3.25,4.0,5.5,6.75\t+\tm6A'


def decline_cases():
    from mcaller_amd import _lib  # noqa: F401
    row = lambda **kw: '\t'.join([kw.get('chrom', 'c'), kw.get('name', 'r'), '7', kw.get('context', 'AAAAAMGAAAA'),     # noqa: E731
                                  kw.get('feats', '1.5,2.5,-3.25,4.0,5.5,6.75'), '+', kw.get('label', 'A')])
    return [
        ('HIGH_BYTE', 1, [GOOD, row(name='réad')], 1),
        ('CONTROL', 2, [GOOD, GOOD, row(name='r\x01ead')], 2),
        ('FIELDS', 3, [GOOD, '', GOOD], 1),
        ('FIELDS', 3, [GOOD, 'c\tr\t7\tAAAAAMGAAAA\t1,2,3,4,5,6\t+'], 1),
        ('PAIR', 4, [GOOD, row(context='CCCCCGGCCCC')], 1),
        ('PAIR', 4, [row(context='AM'), GOOD], 0),
        ('NUMBER', 5, [GOOD, row(feats='1.5,2.5, 3.25,4.0,5.5,6.75')], 1),
        ('NUMBER', 5, [GOOD, row(feats='1.5,2.5,3.25,4.0,5.5,1e400')], 1),
        ('NUMBER', 5, [row(feats='1.5,2.5,3.25,4.0,5.5,3.552713678800501e-16'), GOOD], 0),      # (the residue of a sum that should be zero)
        ('FEATURES', 6, [GOOD, GOOD, row(feats='1.5,2.5,3.25,4.0,5.5,6.75,7.0')], 2),
        ('FEATURES', 6, [row(feats=','.join(['1.5'] * 65))], 0),
        ('CONTEXT', 7, [GOOD, row(context='A' * 32 + 'MG' + 'A' * 31)], 1),
        ('LABELS', 8, [row(label='L%d' % i) for i in range(17)], -1),
        ('LONG_LINE', 9, [GOOD, row(name='R' * 66000)], 1),
    ]


@pytest.mark.parametrize('case', range(14))
def test_declines(tmp_path, case):
    """An ordinary input the device does not reproduce: it says which line and why, and the result -- or the exception -- is the host
    function's.  (Two reasons have no small file: 2^31 - 2 lines, and a text larger than free device memory.)"""
    from mcaller_amd import load_mCaller_data as L
    from mcaller_amd.device import get_device
    name, code, lines, line = decline_cases()[case]
    path = str(tmp_path / 'case.train')
    open(path, 'w', encoding='utf-8', newline='').write('\n'.join(lines) + '\n')
    try:
        host, error = L.tsv2matrix(path, 'A'), None
    except (KeyError, ValueError, IndexError) as e:
        host, error = None, e
    L.last_load = None
    if error is None:
        assert L.tsv2matrix_device(path, 'A') == host
        assert L.last_load['n_rows'] == sum(len(v) for v in host[0]['general'].values())
    else:
        with pytest.raises(type(error)) as got:
            L.tsv2matrix_device(path, 'A')
        assert str(got.value) == str(error)
    st = get_device().training_rows_last_stats()
    assert L.last_load['by'] == 'host' and 'declines' in L.last_load['reason'], L.last_load
    assert (st['decline_reason'], st['decline_line']) == (code, line), (name, st, L.last_load)
    if line >= 0:
        assert '(line %d)' % (line + 1) in L.last_load['reason']


def test_a_long_line_within_the_limit_is_no_decline(tmp_path):
    path = str(tmp_path / 'long.train')
    long_row = GOOD.replace('\tr\t', '\t' + 'R' * 65000 + '\t')
    assert len(long_row) <= 65535
    open(path, 'w').write('\n'.join([GOOD, long_row, GOOD]) + '\n')
    host, dev, load = both(path)
    assert load['by'] == 'device' and T.plain(*dev) == T.plain(*host) and len(dev[0]['general']['m6A']) == 3


def _member_bytes(path):
    blob = open(path, 'rb').read()
    if blob[:2] != b'PK':
        return blob
    with zipfile.ZipFile(path) as z:                          # (a zip's headers carry the time of writing: the members are the model)
        return [(name, z.read(name)) for name in z.namelist()]


@pytest.mark.parametrize('clf', ['NBC', 'LR'])
def test_cli_prints_and_writes_the_same_with_either_reader(tmp_path, monkeypatch, clf):
    from mcaller_amd import load_mCaller_data as L
    from mcaller_amd import mCaller
    td = H.testdata_paths(str(tmp_path))
    rows = str(tmp_path / 'training_rows.train')
    shutil.copy(ROWS, rows)
    monkeypatch.setenv('MCALLER_SEED', '31')
    said, models = [], []
    for knob in (None, '0'):
        if knob is None:
            monkeypatch.delenv('MCALLER_TRAIN_ROWS_DEVICE', raising=False)
        else:
            monkeypatch.setenv('MCALLER_TRAIN_ROWS_DEVICE', knob)
        model = str(tmp_path / ('model_%s_%s.pkl' % (clf, knob)))
        L.last_load = None
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            mCaller.main(['-p', td['test_positions.txt'], '-r', td['fasta'], '-e', td['tsv'], '-f', td['fastq'], '--train',
                          '--training_tsv', rows, '-c', clf, '-d', model])
        assert L.last_load['by'] == ('device' if knob is None else 'host'), L.last_load
        said.append(buf.getvalue())
        models.append(_member_bytes(model))
    assert said[0] == said[1] and 'Cross validation accuracy' in said[0]
    assert models[0] == models[1]


def test_reuse_and_release():
    from mcaller_amd import _lib
    from mcaller_amd.device import get_device
    from mcaller_amd.extract_contexts import base_models
    dev = get_device()
    pairs = sorted(base_models('A', False))
    t1, _ = T.random_file(2, 257)
    t2, _ = T.random_file(5, 513)
    first = dev.training_rows(text=t1, pairs=pairs)
    kept = ([k for k in first[0]], {k: v.copy() for k, v in first[1].items()}, {k: v.copy() for k, v in first[2].items()})
    second = dev.training_rows(text=t2, pairs=pairs)
    assert first[3] is None and second[3] is None
    assert first[0] == kept[0] and all((first[1][k] == kept[1][k]).all() and (first[2][k] == kept[2][k]).all() for k in kept[0])
    _lib.check(_lib.lib().mc_train_rows_release(dev._ctx))
    third = dev.training_rows(text=t1, pairs=pairs)
    assert third[3] is None and third[0] == kept[0]
    assert all(third[1][k].tobytes() == kept[1][k].tobytes() and third[2][k].tolist() == kept[2][k].tolist() for k in kept[0])
    empty = dev.training_rows(text=b'', pairs=pairs)
    assert empty == ([], {}, {}, None)
    dev.training_rows_release()
