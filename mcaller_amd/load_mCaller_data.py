"""`--training_tsv`: labelled `.diffs.<k>.train` rows -> the training dicts.

Same result as the reference's load_mCaller_data.py:3-18 (`tsv2matrix`): per sub-model key and label, the feature rows
and their contexts, in file order.  A label is registered by the first row that carries it (even if that row is left
out); rows with fewer than six features or with a literal `0` feature (an empty slot, written so by
extract_contexts.py:186) are left out.

`tsv2matrix_device` makes the same dicts on the GPU (mcaller_amd/csrc/train/mc_trainrows.hip), with NumPy arrays as leaves: the
device produces exactly what `tsv2matrix` produces, or it declines and `tsv2matrix` does the file."""
import os

from .extract_contexts import base_models


def _usable(fields):
    return len(fields) >= 6 and '0' not in fields


def tsv2matrix(tsvname, base):
    key_of = base_models(base, False)
    signals = {key: {} for key in key_of.values()}
    contexts = {key: {} for key in key_of.values()}
    with open(tsvname, 'r') as rows:
        for row in rows:
            columns = row.split('\t')
            context, features, label = columns[3], columns[4].split(','), columns[6].strip()
            centre = len(context) // 2
            key = key_of[context[centre:centre + 2]]               # KeyError on an unknown pair, like the reference
            by_label = signals[key].setdefault(label, [])
            ctx_by_label = contexts[key].setdefault(label, [])
            if _usable(features):
                by_label.append([float(x) for x in features])
                ctx_by_label.append(context)
    return signals, contexts


last_load = None           # what tsv2matrix_device did last: dict(by='device' | 'host', reason=None | str, n_rows=int)


def tsv2matrix_device(tsvname, base):
    """tsv2matrix with the file read on the GPU (Device.training_rows): the same nesting, {sub-model key: {label: ...}}, with a
    float64 array [n, features] and an 'S' array [n] of contexts as leaves (length 0 for a label whose rows are all left out).
    What the device declines, and everything with MCALLER_TRAIN_ROWS_DEVICE=0, is tsv2matrix's own result -- lists, and the
    reference's exceptions.  `last_load` says who made the matrices."""
    global last_load
    import numpy as np
    key_of = base_models(base, False)
    keys = sorted(set(key_of.values()))
    reason = None
    if os.environ.get('MCALLER_TRAIN_ROWS_DEVICE', '1') == '0':
        reason = 'MCALLER_TRAIN_ROWS_DEVICE=0'
    elif len(keys) != 1:
        reason = 'out of scope on the device: more than one sub-model key'
    else:
        from .device import get_device
        labels, sig, grp, reason = get_device().training_rows(path=tsvname, pairs=sorted(key_of))
    if reason is not None:
        last_load = dict(by='host', reason=reason, n_rows=None)
        signals, contexts = tsv2matrix(tsvname, base)
        last_load['n_rows'] = sum(len(rows) for by_label in signals.values() for rows in by_label.values())
        return signals, contexts
    nf = max([sig[label].shape[1] for label in labels] + [0])
    signals = {keys[0]: {label: sig[label] if len(sig[label]) else np.zeros((0, nf)) for label in labels}}
    contexts = {keys[0]: {label: grp[label] for label in labels}}
    last_load = dict(by='device', reason=None, n_rows=sum(len(sig[label]) for label in labels))
    return signals, contexts
