"""`extract_features` on MI355X: the drop-in for the reference's extract_contexts.py:110-303.

Same signature, same side effects (appends `<tsv minus ext>.diffs.<k>[.train].tmp<startline>`, prints the
five counter lines, returns `(signals, contexts)` in train mode), same error behaviour (messages +
`sys.exit(0)`), but the per-row window machine and the per-observation `predict_proba` run as HIP kernels
behind the C ABI of include/mcaller_hip.h.  The host keeps what is text: FASTA/positions marking
(refmark.py), the model file (model_io.py), context strings and number formatting.

There is no CPU path here: without libmcaller_hip.so or without a GPU every call raises.
"""
import sys

import numpy as np  # noqa: F401  (the names below are this module's as they always were: `from ... import *`, ec.Finisher, ...)

from . import _lib  # noqa: F401
from .device import get_device
from .model_io import load_model_file
from .refmark import MarkedReference, revcomp, strand, base_comps, comp  # noqa: F401  (reference names)
from .rows import (FORMAT_THREADS, Finisher, Prepared, _I, _lookup_quality, base_models, compute, cut_names,  # noqa: F401
                   distinct_positions, fmt_float, head_contig, prepare, prepare_table, round2, submodel_setup, write_text, writefi)
from .stream import (STREAM_MIN_SHARDS, STREAM_SHARD_BYTES, STREAM_SHARD_MAX_BYTES, STREAM_SHARD_MIN_BYTES,  # noqa: F401
                     Clock, PassQueue, RowOutput, ShardFeed, StreamResult, _Unstreamable, shard_schedule, stream_features)


def extract_features(tsv_input, fasta_input, read2qual, k, skip_thresh, qual_thresh, modelfile, classifier,
                     startline, endline=None, train=False, pos_label=None, base=None, motif=None,
                     positions_list=None):
    """Drop-in for extract_contexts.py:110 (see module docstring)."""
    import os
    import time
    timing = os.environ.get('MCALLER_TIMING')
    t_start = time.perf_counter()
    suffix = '.diffs.' + str(k) + ('.train' if train else '') + '.tmp' + str(startline)
    tsv_output = '.'.join(tsv_input.split('.')[:-1]) + suffix                     # :122 / :134
    modelset = None
    if not train:
        modelset = load_model_file(modelfile)                                     # :123-130

    if startline == 0 and endline is not None and os.environ.get('MCALLER_NO_STREAM') is None:
        # a whole file: streamed through the GPU in shards, every shard's rows appended as they come back (:230-232); whatever
        # the shards cannot reproduce (the reference's exit paths, a read name that comes back later) takes the one-table path
        # below from scratch -- the rows appended so far are taken back first, nothing is written or printed twice
        size_before = os.path.getsize(tsv_output) if os.path.exists(tsv_output) else None
        try:
            with open(tsv_output, 'ab') as out_fh:
                res = stream_features(tsv_input, fasta_input, read2qual, k, skip_thresh, qual_thresh, modelset, endline, base,
                                      motif, positions_list, sink=out_fh.write, train=train, pos_label=pos_label)
        except BaseException as e:
            # the rows appended so far are taken back whatever stopped the stream (a device error, MemoryError, ^C: a re-run
            # must not find half a file to append to); only _Unstreamable goes on to the one-table path
            try:                           # (the cleanup must not replace what stopped the stream: the file may never have been opened)
                if size_before is None:
                    os.remove(tsv_output)
                else:
                    os.truncate(tsv_output, size_before)
            except OSError:
                pass
            if not isinstance(e, _Unstreamable):
                raise
        else:
            for line in res.messages:
                print(line)
            counters = res.counters
            if timing:
                ck = getattr(stream_features, 'last_clock', {})
                print('[mcaller_amd timing] streamed in %s shards (%s parsed on the device): total %.3f s | reader / parser threads '
                      '%.3f s | main thread: waiting for the next table %.3f, upload + enqueue %.3f, wait + format %.3f (records '
                      'waited for %.3f, %d records formatted %.3f, %d bytes written %.3f)' % (
                          ck.get('shards'), ck.get('device_parsed'), time.perf_counter() - t_start, ck.get('parse', 0),
                          ck.get('wait_parser', 0), ck.get('enqueue', 0), ck.get('hand_out', 0), ck.get('wait_records', 0),
                          ck.get('records', 0), ck.get('format', 0), ck.get('out_bytes', 0), ck.get('write', 0)), file=sys.stderr)
            if timing == '2':
                for t_ev, what in getattr(stream_features, 'last_clock', {}).get('events', []):
                    print('[mcaller_amd timing] %8.2f ms %s' % (t_ev * 1e3, what), file=sys.stderr)
            for line in counters:                                                 # :295-301
                print(line)
            return (res.signals, res.contexts) if train else None

    P = prepare(tsv_input, fasta_input, read2qual, startline, endline, base, motif, positions_list)
    t_prep = time.perf_counter()
    rec = compute(P, k, skip_thresh, qual_thresh, modelset, base, train)
    t_gpu = time.perf_counter()
    fin = Finisher(P, k, base, train, modelset=modelset, pos_label=pos_label)
    stop = fin.run(rec)
    if stop is None and P.fatal is not None:
        stop = P.fatal
    if stop is not None:
        # the reference dies mid-file: only the 5000-row batches already flushed are on disk (:230-232)
        n_written = (fin.num_observations // 5000) * 5000
        write_text(fin.text(n_written), tsv_output)
        raise stop
    write_text(fin.text(), tsv_output)                                            # :293
    if timing:
        t_end = time.perf_counter()
        print('[mcaller_amd timing] rows=%d records=%d  parse+mark %.3f s | upload+kernels+fetch %.3f s (kernels %s ms) | '
              'format+write %.3f s | total %.3f s' % (P.table.n_rows, rec.n, t_prep - t_start, t_gpu - t_prep,
                                                     get_device().times_ms(), t_end - t_gpu, t_end - t_start),
              file=sys.stderr)

    for line in fin.counters():                                                   # :295-301
        print(line)
    if train:
        return fin.signals, fin.contexts
