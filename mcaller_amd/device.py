"""One MI355X: the resident event table, marked reference, read qualities, classifier, and the hot path."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Params, Records, check, last_error, lib, make_ref_view, _ptr


def default_device_index():
    for var in ('MCALLER_DEVICE', 'LOCAL_RANK'):
        if os.environ.get(var, '') != '':
            return int(os.environ[var])
    return 0


def _serialized(fn):
    """A method that calls the library on the context: one at a time (the C ABI's contract)."""
    import functools

    @functools.wraps(fn)
    def call(self, *a, **kw):
        with self._lock:
            return fn(self, *a, **kw)
    return call


def _contig_table(contigs):
    """compare_genomes.read_fai's (names, lens, offs) as a mc_contig_table -> (the struct, what its pointers point at)."""
    names, _, offs = contigs
    ids = [name.encode('utf-8', 'surrogateescape') for name in names]
    id_off = np.zeros(len(ids) + 1, dtype=np.int64)
    id_off[1:] = np.cumsum([len(i) for i in ids], dtype=np.int64)
    pool = np.frombuffer(b''.join(ids) + b'\0', dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    t = _lib.ContigTable()
    t.n_contigs = len(ids)
    t.ids, t.id_off, t.off = _ptr(pool), _ptr(id_off), _ptr(offs)
    return t, (pool, id_off, offs)


def _source(path=None, text=None):
    """A file (`path`) or a text (`text`, bytes) as a mc_text_source -> (what a call takes: a reference to the struct, or None
    without either; what the call reads from)."""
    if path is None and text is None:
        return None, None
    keep = os.fsencode(path) if path is not None else bytes(text)
    s = _lib.TextSource()
    if path is not None:
        s.path = C.cast(C.c_char_p(keep), C.c_void_p)
    else:
        s.text, s.n_bytes = C.cast(C.c_char_p(keep), C.c_void_p), len(keep)
    return C.byref(s), (s, keep)


def _blob(ptr, n):
    """The n bytes a call handed out at `ptr`, as the caller's own copy (no bytes: b'', whatever the pointer)."""
    return C.string_at(ptr, n) if n else b''


def _first_row_columns(path=None, text=None):
    """c, the value columns of a .diffs file (`path`) or text (`text`, bytes), from its first row: the values of a row less the
    read quality (0: the row has not 7 or 8 fields)."""
    if path is not None:
        with open(path, 'rb') as fh:
            first = fh.readline()
    else:
        first = bytes(text).split(b'\n', 1)[0]
    fields = first.split(b'\t')
    return fields[4].count(b',') if len(fields) in (7, 8) else 0


class Device(object):
    def __init__(self, index=None):
        import threading
        self._lock = threading.RLock()      # calls on a context are serialized (include/mcaller_hip.h): the stream's formatter thread scores a stray record while the main thread waits
        self.index = default_device_index() if index is None else int(index)
        self._ctx = C.c_void_p()
        check(lib().mc_ctx_create(self.index, C.byref(self._ctx)))
        self._keep = {}

    @staticmethod
    def bind_host_to_numa_node(device):
        """One process per GPU: bind this process to the cores next to `device` (-> NUMA node, or -1: unknown, unchanged)."""
        return int(lib().mc_bind_to_device_numa_node(int(device)))

    def close(self):
        with self._lock:
            if self._ctx:
                lib().mc_ctx_destroy(self._ctx)
                self._ctx = C.c_void_p()

    def _row_text_release(self, block):
        """A RowText gives its pinned block back (any thread; nothing to do once the context is gone)."""
        with self._lock:
            if self._ctx:
                lib().mc_row_text_release(self._ctx, int(block))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _last_stats(self, fn, struct):
        """A *_last_stats call of the library as a dict of the struct's fields (padding left out)."""
        st = struct()
        check(fn(self._ctx, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_ if not name.startswith('pad')}

    # ---- resident inputs ----
    @_serialized
    def set_reference(self, arrays):
        v = make_ref_view(arrays)
        check(lib().mc_ctx_set_reference(self._ctx, C.byref(v)))

    @_serialized
    def set_reference_motif(self, arrays, motif_fwd, repl_fwd, motif_rev, repl_rev):
        """The reference from its raw bases, site masks made on the GPU (arrays: MarkedReference.raw_arrays(); motifs:
        MarkedReference.motif_for_the_device())."""
        v = _lib.make_ref_view(arrays)
        v.n_words = int(arrays['n_words'])
        check(lib().mc_ctx_set_reference_motif(self._ctx, C.byref(v), motif_fwd, repl_fwd, len(motif_fwd), motif_rev, repl_rev,
                                               len(motif_rev)))

    @_serialized
    def set_reference_iupac(self, arrays, spec):
        """The same for a set of degenerate motifs (arrays: MarkedReference.raw_arrays(); spec: MarkedReference.iupac_for_the_device(),
        an _lib.IupacSpec)."""
        v = _lib.make_ref_view(arrays)
        v.n_words = int(arrays['n_words'])
        check(lib().mc_ctx_set_reference_iupac(self._ctx, C.byref(v), C.byref(spec)))

    @_serialized
    def fetch_reference(self, n_seq_bytes, n_words, n_contigs):
        """(seq, mbits_fwd, mbits_rev, rank_fwd, rank_rev, site_base, n_sites) as the device holds them (tests)."""
        seq = np.empty(n_seq_bytes, dtype=np.uint8)
        mf, mr = np.empty(n_words, dtype=np.uint32), np.empty(n_words, dtype=np.uint32)
        rf, rr = np.empty(n_words, dtype=np.int32), np.empty(n_words, dtype=np.int32)
        base, n_sites = np.empty(2 * n_contigs, dtype=np.int64), C.c_int64(0)
        check(lib().mc_ctx_fetch_reference(self._ctx, _ptr(seq), int(n_seq_bytes), _ptr(mf), _ptr(mr), _ptr(rf), _ptr(rr), int(n_words),
                                           _ptr(base), C.byref(n_sites)))
        return seq, mf, mr, rf, rr, base, n_sites.value

    @_serialized
    def upload_table(self, table):
        v = table.view()
        check(lib().mc_ctx_upload_table(self._ctx, C.byref(v)))
        self.n_rows = table.n_rows
        return self.current_slot()

    @_serialized
    def current_slot(self):
        return int(lib().mc_ctx_current_slot(self._ctx))

    @_serialized
    def select_table(self, slot, as_new=False):
        """Make the table resident in `slot` the current one again; as_new: the next pass does everything the first pass over a
        table does (every row validated), whatever earlier passes learned about it."""
        check(lib().mc_ctx_select_table(self._ctx, int(slot), 1 if as_new else 0))

    @_serialized
    def reserve_tables(self, max_rows, max_segs, max_reads):
        """Size the table slots, the per-pass scratch and the record sets once for a stream of tables up to these sizes."""
        check(lib().mc_ctx_reserve_tables(self._ctx, int(max_rows), int(max_segs), int(max_reads)))

    @_serialized
    def upload_table_async(self, table, qual=None):
        """Enqueue the upload of `table` (+ its read qualities) into a free slot and make it the current table; returns the
        slot.  The table's arrays must stay alive and untouched until wait_upload(slot) (or until the records of a pass over
        it have been handed out); they should be pinned (Table.pinned(), or parsed with the pool switched on)."""
        q = None if qual is None else np.ascontiguousarray(qual, dtype=np.float64)
        if getattr(table, 'device_slot', None) is not None:          # parsed on the device: the columns are in the slot already
            sr = np.ascontiguousarray(table.seg_read, dtype=np.int32)
            check(lib().mc_ctx_parse_finish(self._ctx, int(table.device_slot), _ptr(sr), int(table.n_reads),
                                            None if q is None else _ptr(q)))
            self.n_rows = table.n_rows
            slot, table.device_slot = table.device_slot, None
            return slot
        v = table.view()
        slot = C.c_int32(-1)
        check(lib().mc_ctx_upload_table_async(self._ctx, C.byref(v), None if q is None else _ptr(q), C.byref(slot)))
        self.n_rows = table.n_rows
        return slot.value

    # ---- the eventalign text parsed on the device (mc_ctx_parse_*) ----
    @_serialized
    def parse_begin(self, text, contig_names, max_rows):
        """Send a TextBlock and enqueue the parse into a free table slot -> slot."""
        arr = (C.c_char_p * max(1, len(contig_names)))()
        for i, n in enumerate(contig_names):
            arr[i] = n.encode('utf-8')
        slot = C.c_int32(-1)
        check(lib().mc_ctx_parse_begin(self._ctx, text.ptr, int(text.n_bytes), arr, len(contig_names), int(max_rows), C.byref(slot)))
        return slot.value

    @_serialized
    def parse_end(self, slot, text):
        """-> the Table (columns on the device, in `slot`; upload_table_async finishes it), or None: the shard needs the host
        parser (the slot has been given back)."""
        res = _lib.DevParseResult()
        check(lib().mc_ctx_parse_end(self._ctx, int(slot), C.byref(res)))
        if res.status != 0:
            self.parse_fallback_reason = last_error()
            check(lib().mc_ctx_parse_abandon(self._ctx, int(slot)))
            return None
        t = _lib.device_table(res, text)
        t.device_slot = int(slot)
        return t

    @_serialized
    def parse_abandon(self, slot):
        check(lib().mc_ctx_parse_abandon(self._ctx, int(slot)))

    @_serialized
    def fetch_columns(self, slot, n_rows):
        """(pos, evmu [n, 2], event_idx, flags) of the table in `slot`, copied back (tests)."""
        pos, evmu = np.empty(n_rows, dtype=np.int32), np.empty((n_rows, 2), dtype=np.int32)
        idx, fl = np.empty(n_rows, dtype=np.int32), np.empty(n_rows, dtype=np.uint8)
        check(lib().mc_ctx_fetch_columns(self._ctx, int(slot), int(n_rows), _ptr(pos), _ptr(evmu), _ptr(idx), _ptr(fl)))
        return pos, evmu, idx, fl

    @_serialized
    def fetch_model_n_bits(self, slot, n_rows):
        """The model-N bit column of the table in `slot`, ceil(n_rows / 8) bytes, the bits at or beyond n_rows cleared (tests)."""
        out = np.zeros((n_rows + 7) // 8 + 1, dtype=np.uint8)
        check(lib().mc_ctx_fetch_model_n_bits(self._ctx, int(slot), int(n_rows), _ptr(out)))
        out = out[:(n_rows + 7) // 8]
        if n_rows % 8:
            out[-1] &= (1 << (n_rows % 8)) - 1
        return out

    @_serialized
    def fetch_idx_rel_bits(self, slot, n_rows):
        """The index-relation column of the table in `slot`, ceil(n_rows / 8) uint16, the bits at or beyond n_rows cleared (tests)."""
        out = np.zeros((n_rows + 7) // 8 + 1, dtype=np.uint16)
        check(lib().mc_ctx_fetch_idx_rel_bits(self._ctx, int(slot), int(n_rows), _ptr(out)))
        out = out[:(n_rows + 7) // 8]
        if n_rows % 8:
            out[-1] &= ((1 << (n_rows % 8)) - 1) * 0x0101
        return out

    @_serialized
    def fetch_pos_rel_bits(self, slot, n_rows):
        """The position-relation column of the table in `slot`, ceil(n_rows / 8) uint16 (tests)."""
        out = np.zeros((n_rows + 7) // 8 + 1, dtype=np.uint16)
        check(lib().mc_ctx_fetch_pos_rel_bits(self._ctx, int(slot), int(n_rows), _ptr(out)))
        return out[:(n_rows + 7) // 8]

    @_serialized
    def fetch_unit_summaries(self, slot, n_rows):
        """The unit summaries of the table in `slot`, [ceil(n_rows / 8), 2] int32: first and last position of every unit of eight
        rows; the second of a last, partial unit is unspecified (tests)."""
        out = np.zeros(((n_rows + 7) // 8 + 1, 2), dtype=np.int32)
        check(lib().mc_ctx_fetch_unit_summaries(self._ctx, int(slot), int(n_rows), _ptr(out)))
        return out[:(n_rows + 7) // 8]

    @_serialized
    def wait_upload(self, slot):
        check(lib().mc_ctx_wait_upload(self._ctx, int(slot)))

    @_serialized
    def upload_times_ms(self, slot):
        """(H2D ms, 0.0) of the last upload into `slot`; waits for it.  (Nothing runs at upload: the first pass validates.)"""
        a, b = C.c_float(0), C.c_float(0)
        check(lib().mc_ctx_upload_times_ms(self._ctx, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    @_serialized
    def parse_times_ms(self, slot):
        """(text H2D ms, device parser ms) of the parse begun into `slot` (between parse_begin and parse_end / parse_abandon)."""
        a, b = C.c_float(0), C.c_float(0)
        check(lib().mc_ctx_parse_times_ms(self._ctx, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    @_serialized
    def set_read_quality(self, qual):
        q = np.ascontiguousarray(qual, dtype=np.float64)
        check(lib().mc_ctx_set_read_quality(self._ctx, _ptr(q), len(q)))

    @_serialized
    def set_mlp(self, weights, submodel_of_char):
        """weights: list of MLPWeights (same shapes); submodel_of_char: uint8[256]."""
        n_in, n_hidden = weights[0].n_in, weights[0].n_hidden
        for w in weights:
            if (w.n_in, w.n_hidden) != (n_in, n_hidden):
                raise NotImplementedError('sub-models with different shapes')
        W1 = np.ascontiguousarray(np.stack([w.W1 for w in weights]), dtype=np.float64)
        b1 = np.ascontiguousarray(np.stack([w.b1 for w in weights]), dtype=np.float64)
        W2 = np.ascontiguousarray(np.stack([w.W2 for w in weights]), dtype=np.float64)
        b2 = np.ascontiguousarray(np.concatenate([w.b2 for w in weights]), dtype=np.float64)
        soc = np.ascontiguousarray(submodel_of_char, dtype=np.uint8)
        assert soc.shape == (256,)
        check(lib().mc_ctx_set_mlp(self._ctx, len(weights), n_in, n_hidden, _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2),
                                   _ptr(soc)))

    @_serialized
    def set_forest(self, forests, submodel_of_char):
        """forests: list of ForestWeights (one per sub-model)."""
        arr = forest_arrays(forests)
        soc = np.ascontiguousarray(submodel_of_char, dtype=np.uint8)
        check(lib().mc_ctx_set_forest(self._ctx, len(forests), forests[0].n_in, _ptr(arr['model_tree_off']),
                                      _ptr(arr['tree_node_off']), _ptr(arr['left']), _ptr(arr['right']),
                                      _ptr(arr['feature']), _ptr(arr['threshold']), _ptr(arr['value']), _ptr(soc)))
        self._clf = 'forest'

    @_serialized
    def set_simple(self, models, submodel_of_char):
        """models: list of LogisticWeights or of GaussianNBWeights (one per sub-model) -- `-c LR` / `-c NBC`."""
        kind = {'logistic': 1, 'gnb': 2}[models[0].kind]
        if any(m.kind != models[0].kind or m.n_in != models[0].n_in for m in models):
            raise NotImplementedError('sub-models of different kinds or shapes')
        params = np.ascontiguousarray(np.stack([m.params() for m in models]), dtype=np.float64)
        soc = np.ascontiguousarray(submodel_of_char, dtype=np.uint8)
        check(lib().mc_ctx_set_simple_classifier(self._ctx, kind, len(models), models[0].n_in, _ptr(params), params.shape[1], _ptr(soc)))
        self._clf = 'simple'

    @_serialized
    def set_svm(self, models, submodel_of_char):
        """models: list of SVMWeights (one per sub-model, support-vector counts of their own) -- `-c SVM`."""
        if any(m.n_in != models[0].n_in for m in models):
            raise NotImplementedError('sub-models of different shapes')
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([m.n_sv for m in models])]), dtype=np.int32)
        sv = np.ascontiguousarray(np.concatenate([m.sv for m in models]), dtype=np.float64)
        coef = np.ascontiguousarray(np.concatenate([m.dual_coef for m in models]), dtype=np.float64)
        params = np.ascontiguousarray(np.stack([m.params() for m in models]), dtype=np.float64)
        soc = np.ascontiguousarray(submodel_of_char, dtype=np.uint8)
        check(lib().mc_ctx_set_svm(self._ctx, len(models), models[0].n_in, _ptr(off), _ptr(sv), _ptr(coef), _ptr(params), _ptr(soc)))
        self._clf = 'svm'

    def set_classifier(self, weights, submodel_of_char):
        """MLP, forest, logistic regression, naive Bayes or RBF SVM, whatever the model file held (extract_contexts.py:199 calls
        any of them the same way)."""
        if weights[0].kind == 'forest':
            self.set_forest(weights, submodel_of_char)
        elif weights[0].kind in ('logistic', 'gnb'):
            self.set_simple(weights, submodel_of_char)
        elif weights[0].kind == 'svm':
            self.set_svm(weights, submodel_of_char)
        else:
            self.set_mlp(weights, submodel_of_char)
            self._clf = 'mlp'

    @_serialized
    def classifier_forward(self, X, submodel):
        X = np.ascontiguousarray(X, dtype=np.float64)
        sm = np.ascontiguousarray(submodel, dtype=np.uint8)
        p = np.empty(len(X), dtype=np.float64)
        fn = {'forest': lib().mc_forest_forward, 'simple': lib().mc_simple_forward,
              'svm': lib().mc_svm_forward}.get(getattr(self, '_clf', 'mlp'), lib().mc_mlp_forward)
        check(fn(self._ctx, _ptr(X), _ptr(sm), len(X), _ptr(p)))
        return p

    # ---- the hot path ----
    @_serialized
    def run(self, k, skip_thresh, qual_thresh, tail_contig=-1, score=True, entry_read=-1, entry_first_idx=0):
        """K0+K1+K2 on the resident table; records stay on the device.  Returns their number."""
        p = Params(int(k), int(skip_thresh), float(qual_thresh), int(tail_contig), 1 if score else 0,
                   int(entry_read), int(entry_first_idx))
        n = C.c_int64(0)
        check(lib().mc_extract_features(self._ctx, C.byref(p), C.byref(n)))
        self._last = (n.value, int(k))
        return n.value

    @_serialized
    def run_async(self, k, skip_thresh, qual_thresh, tail_contig=-1, score=True, entry_read=-1, entry_first_idx=0):
        """Enqueue one pass (K0 + K1 on the ctx stream, the emit, K2 + packing on a side stream); at most six in flight."""
        p = Params(int(k), int(skip_thresh), float(qual_thresh), int(tail_contig), 1 if score else 0,
                   int(entry_read), int(entry_first_idx))
        check(lib().mc_extract_features_async(self._ctx, C.byref(p)))
        self._async_k = getattr(self, '_async_k', []) + [int(k)]

    @_serialized
    def wait_begin(self):
        """Start the copy-out of the oldest pass whose copy-out has not been started, without waiting for it."""
        check(lib().mc_wait_records_begin(self._ctx))

    @_serialized
    def wait(self):
        """Records of the oldest pass in flight: views of pinned buffers (slot means / probabilities of the calls only, see
        Records.call_row), valid until six more passes have been enqueued."""
        n, v = C.c_int64(0), _lib.CallsView()
        check(lib().mc_wait_records(self._ctx, C.byref(n), C.byref(v)))
        k = self._async_k.pop(0)
        self._last = (n.value, k)
        rerun = C.c_int32(0)
        check(lib().mc_last_pass_info(self._ctx, None, C.byref(rerun)))
        if rerun.value:
            # a pass the library repeated synchronously (irregular reads, record buffers too small) hands out the context's ONE set
            # of buffers for synchronous runs, which the next such pass overwrites -- and the stream's formatter thread reads a
            # shard's records while the main thread waits for the next pass: such records are copied (they are rare)
            rec = Records(n.value, k)
            vc = rec.view()
            check(lib().mc_fetch_records(self._ctx, C.byref(vc)))
            rec.n = n.value
            return rec
        rec = Records.from_view(v, n.value, k, self)
        text, nb, nr, block = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int32(-1)
        check(lib().mc_last_row_text(self._ctx, C.byref(text), C.byref(nb), C.byref(nr), C.byref(block)))
        if block.value >= 0:                 # the rows as text, made on the device (row_text): the host formatter has nothing to do
            rec.row_text = _lib.RowText(self, text.value, nb.value, nr.value, block.value)
        return rec

    @_serialized
    def row_text(self, on, label_meth=None, label_unmeth=None, first=False):
        """The passes enqueued from now on also write their rows as text on the device (mc_ctx_row_text): wait() hands them out as
        Records.row_text when the pass had them.  first: the start of a stream -- blocks an earlier stream never gave back are taken
        back (nobody reads them any more)."""
        check(lib().mc_ctx_row_text(self._ctx, (2 if first else 1) if on else 0, label_meth.encode() if label_meth else None,
                                    label_unmeth.encode() if label_unmeth else None))

    ROWTEXT_PROBE_STRIDE = 48            # MC_ROWTEXT_PROBE_STRIDE
    ROWTEXT_PROBE_FILL = 0xA5

    @_serialized
    def rowtext_probe(self, values=(), fixed=(), prob=(), shift=0):
        """The row writer's numbers alone (mc_ctx_rowtext_probe, tests): doubles through the digit kernel (the first half as wide slot
        means, the rest as read qualities), int32 slot means as repr(d / 1e4), probabilities as np.round(p, 2).  -> (text: uint8
        [items, ROWTEXT_PROBE_STRIDE], item i written from byte (i + shift) % 8 of its line; counted lengths (-1: not printed); ok)."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        f = np.ascontiguousarray(fixed, dtype=np.int32)
        p = np.ascontiguousarray(prob, dtype=np.float64)
        n_all = len(v) + len(f) + len(p)
        text = np.empty((n_all, self.ROWTEXT_PROBE_STRIDE), dtype=np.uint8)
        length = np.empty(n_all, dtype=np.int32)
        ok = np.empty(n_all, dtype=np.uint8)
        check(lib().mc_ctx_rowtext_probe(self._ctx, _ptr(v), len(v), _ptr(f), len(f), _ptr(p), len(p), int(shift), _ptr(text), _ptr(length),
                                         _ptr(ok)))
        return text, length, ok.astype(bool)

    @_serialized
    def fetch(self, copy=True):
        """Records of the last run.  copy=False: views of the context's pinned buffers (overwritten by the next run)."""
        n, k = self._last
        if not copy:
            v = _lib.CallsView()
            check(lib().mc_fetch_records_view(self._ctx, C.byref(v)))
            return Records.from_view(v, n, k, self)
        rec = Records(n, k)
        v = rec.view()
        check(lib().mc_fetch_records(self._ctx, C.byref(v)))
        rec.n = n
        return rec

    def extract(self, k, skip_thresh, qual_thresh, **kw):
        self.run(k, skip_thresh, qual_thresh, **kw)
        return self.fetch()

    @_serialized
    def sync(self):
        """hipDeviceSynchronize on this context's device (all of its streams)."""
        check(lib().mc_ctx_sync(self._ctx))

    @_serialized
    def set_pass_timing(self, every_n):
        """Pipelined passes: record the timing events with every n-th pass only (each costs the queue ~9 us); 0 = never."""
        check(lib().mc_ctx_set_pass_timing(self._ctx, int(every_n)))

    @_serialized
    def last_pass_timed(self):
        return bool(lib().mc_last_pass_timed(self._ctx))

    @_serialized
    def last_pass_info(self):
        """(record slots per piece if the pass handed out last ran as the fused dense kernel, else 0; whether it was repeated
        synchronously inside wait())."""
        a, b = C.c_int32(0), C.c_int32(0)
        check(lib().mc_last_pass_info(self._ctx, C.byref(a), C.byref(b)))
        return a.value, bool(b.value)

    @_serialized
    def last_scan_mode(self):
        """What the scan of the pass enqueued last streams (mc_ctx_last_scan_mode): 0 the columns, validating; 1 the columns;
        2 unit summaries; 3 unit summaries and the relation columns, validating (tests)."""
        return int(lib().mc_ctx_last_scan_mode(self._ctx))

    @_serialized
    def whole_tiles(self, n_rows):
        """A bool per tile of 2048 rows of the current table (n_rows rows): the scan that streams unit summaries takes the tile in
        a single batch -- its own predicate on the descriptors of the synchronous pass run last (mc_ctx_whole_tiles; tests)."""
        out = np.zeros((n_rows + 2047) // 2048, dtype=np.uint8)
        n = int(lib().mc_ctx_whole_tiles(self._ctx, _ptr(out)))
        check(min(n, 0))
        assert n == int(out.sum())
        return out.astype(bool)

    @_serialized
    def times_ms(self):
        t = np.zeros(5, dtype=np.float32)
        check(lib().mc_last_times_ms(self._ctx, _ptr(t)))
        return dict(strand_resolve=float(t[0]), window_scan=float(t[1]), emit=float(t[2]), classifier=float(t[3]),
                    total=float(t[4]))

    # ---- per-site reduction feeding make_bed (the one exchange step of a multi-GPU job) ----
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId (call on rank 0, ship the 128 bytes to every rank)."""
        buf = np.zeros(128, dtype=np.uint8)
        check(lib().mc_comm_unique_id(_ptr(buf)))
        return buf.tobytes()

    @staticmethod
    def comm_probe():
        """Can librccl.so be loaded in this process?  Raises if not (nothing else is touched)."""
        check(lib().mc_comm_available())

    @_serialized
    def site_counts_fetch(self):
        """This rank's own per-site counts as they stand (no collective) -> (n_meth, n_total, first)."""
        n = lib().mc_site_count(self._ctx)
        n_meth, n_total = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        first = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
        check(lib().mc_site_counts_fetch(self._ctx, _ptr(n_meth), _ptr(n_total), _ptr(first)))
        return n_meth, n_total, first

    @_serialized
    def comm_init(self, world, rank, unique_id):
        """ncclCommInitRank on this GPU (RCCL over xGMI); collective over all ranks."""
        uid = np.frombuffer(unique_id, dtype=np.uint8).copy()
        assert len(uid) == 128
        check(lib().mc_comm_init(self._ctx, int(world), int(rank), _ptr(uid)))

    @_serialized
    def comm_destroy(self):
        lib().mc_comm_destroy(self._ctx)

    @_serialized
    def site_counts(self, row_offset=0, tail_contig=-1):
        """Per-site counts of the last run's records, on the device.  Returns how many records the host scored itself
        (NaN probability on the device): add those with site_counts_add.  Records closed by a row of another contig than
        their site's are left out too (self.n_cross_contig; make_bed.cross_contig_records lists them)."""
        pending, cross = C.c_int64(0), C.c_int64(0)
        check(lib().mc_site_counts(self._ctx, int(row_offset), int(tail_contig), C.byref(pending), C.byref(cross)))
        self.n_cross_contig = cross.value
        return pending.value

    @_serialized
    def site_counts_reset(self):
        """Zero the device-side per-site counts (before the first shard of a streamed file)."""
        check(lib().mc_site_counts_reset(self._ctx))

    @_serialized
    def site_counts_accumulate(self, row_offset=0, tail_contig=-1):
        """Add the records of the pass handed out last to the per-site counts (a streamed file: shard after shard); returns
        like site_counts."""
        pending, cross = C.c_int64(0), C.c_int64(0)
        check(lib().mc_site_counts_accumulate(self._ctx, int(row_offset), int(tail_contig), C.byref(pending), C.byref(cross)))
        self.n_cross_contig = cross.value
        return pending.value

    @_serialized
    def site_counts_add(self, site, is_meth, first_row):
        site = np.ascontiguousarray(site, dtype=np.int64)
        meth = np.ascontiguousarray(is_meth, dtype=np.uint8)
        first = np.ascontiguousarray(first_row, dtype=np.int64)
        check(lib().mc_site_counts_add(self._ctx, _ptr(site), _ptr(meth), _ptr(first), len(site)))

    @_serialized
    def site_allreduce(self):
        """Sum / min over the ranks of the communicator (none: this rank alone) -> (n_meth, n_total, first, ms)."""
        n = lib().mc_site_count(self._ctx)
        n_meth, n_total = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        first = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
        ms = C.c_float(0)
        check(lib().mc_site_allreduce(self._ctx, _ptr(n_meth), _ptr(n_total), _ptr(first), C.byref(ms)))
        return n_meth, n_total, first, ms.value

    # ---- the classifier fit behind --train ----
    @staticmethod
    def _fit_jobs(X, y, jobs, who=None, need_spread=False):
        """X, y and a fit's jobs [(train_rows, validation_rows)] as the C ABI takes them -> (X, y, tr, va, tr_off, va_off, tr_idx,
        va_idx): the jobs' index arrays, their offsets and their concatenations (one spare entry at the end, so that neither is
        empty).  With `who` (svm_fit, lr_fit, nb_fit) the call is validated first, a ValueError in that name: finite X of 1..64
        features, y in {0, 1}, per job two training rows of both classes, every index a row of X and, for need_spread, training rows
        that are not all equal."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        if who:
            if X.ndim != 2 or not 1 <= X.shape[1] <= 64 or len(y) != len(X):
                raise ValueError('%s: X must be rows x 1..64 features with a label per row, got %s and %d labels' % (who, X.shape, len(y)))
            if not np.isfinite(X).all() or (y > 1).any():
                raise ValueError('%s: X must be finite and y in {0, 1}' % who)
            if len(jobs) < 1:
                raise ValueError('%s: at least one job is needed' % who)
        n = len(X)
        tr = [np.ascontiguousarray(j[0], dtype=np.int32) for j in jobs]
        va = [np.ascontiguousarray(j[1], dtype=np.int32) for j in jobs]
        if who:
            for a, b in zip(tr, va):
                if len(a) < 2 or (a < 0).any() or (a >= n).any() or (b < 0).any() or (b >= n).any():
                    raise ValueError('%s: every job needs two training rows, every index within the %d rows' % (who, n))
                if len(np.unique(y[a])) != 2:
                    raise ValueError('%s: a job whose training rows are of one class' % who)
                if need_spread and np.ptp(X[a], axis=0).max() == 0:
                    raise ValueError('%s: a job whose training rows are all equal (epsilon_ = 0: every variance would be 0)' % who)
        tr_off = np.concatenate([[0], np.cumsum([len(a) for a in tr])]).astype(np.int64)
        va_off = np.concatenate([[0], np.cumsum([len(a) for a in va])]).astype(np.int64)
        tr_idx = np.ascontiguousarray(np.concatenate(tr + [np.zeros(1, np.int32)]))
        va_idx = np.ascontiguousarray(np.concatenate(va + [np.zeros(1, np.int32)]))
        return X, y, tr, va, tr_off, va_off, tr_idx, va_idx

    @_serialized
    def mlp_fit(self, X, y, jobs, hidden=100, alpha=0.001, lr_init=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8,
                batch_size=200, max_iter=200, tol=1e-4, n_iter_no_change=10, shuffle=True, seed=1, seeds=None, init=None):
        """Fit one 7-H-1 tanh/logistic perceptron per job on the GPU (mc_mlp_fit; all jobs side by side).
        jobs: [(train_rows, validation_rows)] index arrays into X / y.  -> list of dicts W1, b1, W2, b2, loss_curve,
        n_iter, val_correct, n_val."""
        X, y, tr, va, tr_off, va_off, tr_idx, va_idx = self._fit_jobs(X, y, jobs)
        n, d = X.shape
        nj = len(jobs)
        prm = _lib.FitParams(d, int(hidden), int(batch_size), int(max_iter), int(n_iter_no_change), 1 if shuffle else 0,
                             float(alpha), float(lr_init), float(beta1), float(beta2), float(epsilon), float(tol), int(seed))
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        ini = None
        if init is not None:      # [(W1, b1, W2, b2)] per job
            ini = np.ascontiguousarray(np.concatenate([np.concatenate([np.ravel(w[0]), np.ravel(w[1]), np.ravel(w[2]),
                                                                       np.ravel([w[3]])]) for w in init]), dtype=np.float64)
            assert len(ini) == nj * (d * hidden + 2 * hidden + 1)
        W1 = np.zeros((nj, d, hidden)); b1 = np.zeros((nj, hidden)); W2 = np.zeros((nj, hidden)); b2 = np.zeros(nj)
        curve = np.zeros((nj, max_iter)); n_iter = np.zeros(nj, dtype=np.int32); correct = np.zeros(nj, dtype=np.int64)
        check(lib().mc_mlp_fit(self._ctx, C.byref(prm), _ptr(X), _ptr(y), n, nj, _ptr(tr_off), _ptr(tr_idx), _ptr(va_off),
                               _ptr(va_idx), None if sd is None else _ptr(sd), None if ini is None else _ptr(ini),
                               _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(curve), _ptr(n_iter), _ptr(correct)))
        return [dict(W1=W1[j], b1=b1[j], W2=W2[j], b2=float(b2[j]), loss_curve=curve[j, :n_iter[j]].copy(),
                     n_iter=int(n_iter[j]), val_correct=int(correct[j]), n_val=len(va[j])) for j in range(nj)]

    @_serialized
    def forest_fit(self, X, y, jobs, n_trees=50, max_depth=10, max_features=4, min_samples_split=3, min_samples_leaf=2,
                   bootstrap=True, seed=1, seeds=None):
        """Fit one random forest per job on the GPU (mc_forest_fit: every tree of every job side by side; scikit-learn's
        RandomForestClassifier(criterion='entropy') with keyed randomness).  jobs: [(train_rows, validation_rows)] index arrays into
        X / y (y in {0, 1}).  -> per job a dict: tree_off [n_trees+1], the node arrays of its trees concatenated (left, right local
        to each tree; feature, threshold, value [n, 2], impurity, n_node_samples, weighted_n_node_samples), val_correct, n_val."""
        X, y, tr, va, tr_off, va_off, tr_idx, va_idx = self._fit_jobs(X, y, jobs)
        n, d = X.shape
        if max_features > d:
            raise ValueError('max_features must be in (0, n_features]: %d > %d' % (max_features, d))
        nj = len(jobs)
        sd = np.ascontiguousarray([(seed + j) % (1 << 64) for j in range(nj)] if seeds is None else seeds, dtype=np.uint64)
        max_tr = max(len(a) for a in tr)
        m = np.arange(max_tr + 1, dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            G = m * np.log(m)                                     # G[m] = m ln m: both sides read these bits
        G[0] = 0.0
        cap = sum(int(n_trees) * min((2 << int(max_depth)) - 1, max(2 * len(a) - 1, 1)) for a in tr)
        prm = _lib.ForestParams(d, int(n_trees), int(max_depth), int(max_features), int(min_samples_split), int(min_samples_leaf),
                                1 if bootstrap else 0)
        toff = np.zeros(nj * n_trees + 1, dtype=np.int64)
        left = np.empty(cap, np.int32); right = np.empty(cap, np.int32); feature = np.empty(cap, np.int32)
        threshold = np.empty(cap); value = np.empty((cap, 2)); impurity = np.empty(cap)
        n_node = np.empty(cap, np.int32); weighted = np.empty(cap); correct = np.zeros(nj, dtype=np.int64)
        check(lib().mc_forest_fit(self._ctx, C.byref(prm), _ptr(X), _ptr(y), n, nj, _ptr(tr_off), _ptr(tr_idx), _ptr(va_off),
                                  _ptr(va_idx), _ptr(sd), _ptr(G), len(G), cap, _ptr(toff), _ptr(left), _ptr(right), _ptr(feature),
                                  _ptr(threshold), _ptr(value), _ptr(impurity), _ptr(n_node), _ptr(weighted), _ptr(correct)))
        out = []
        for j in range(nj):
            a, b = toff[j * n_trees], toff[(j + 1) * n_trees]
            out.append(dict(tree_off=toff[j * n_trees:(j + 1) * n_trees + 1] - a, left=left[a:b].copy(), right=right[a:b].copy(),
                            feature=feature[a:b].copy(), threshold=threshold[a:b].copy(), value=value[a:b].copy(),
                            impurity=impurity[a:b].copy(), n_node_samples=n_node[a:b].copy(),
                            weighted_n_node_samples=weighted[a:b].copy(), val_correct=int(correct[j]), n_val=len(va[j])))
        return out

    @_serialized
    def forest_fit_last_stats(self):
        """How the last forest_fit ran (mc_forest_fit_stats): n_batches launches of `batch` trees each (what fits
        MCALLER_FOREST_MEM_MB at per_tree_bytes a tree), n_trees_total, n_nodes."""
        return self._last_stats(lib().mc_forest_fit_last_stats, _lib.ForestFitStats)

    @_serialized
    def svm_fit(self, X, y, jobs, gammas, C=1.0, tol=1e-3, max_iter=0):
        """Solve one RBF SVC dual per job on the GPU (mc_svm_fit: every job a workgroup of k6_svm_fit, libsvm's Solver).  jobs:
        [(train_rows, validation_rows)] index arrays into X / y (y in {0, 1}); a job's training rows come in libsvm's solve order,
        the class of its first row being the solve's +1.  -> per job a dict: alpha (per training row), rho, n_iter, status (1: the
        iteration cap was reached), val_dec (> 0: class 0), val_correct, n_val."""
        X, y, tr, va, tr_off, va_off, tr_idx, va_idx = self._fit_jobs(X, y, jobs, 'svm_fit')
        n, d = X.shape
        nj = len(jobs)
        g = np.ascontiguousarray(gammas, dtype=np.float64)
        if len(g) != nj or not (np.isfinite(g) & (g > 0)).all():
            raise ValueError('svm_fit: a finite gamma > 0 per job is needed')
        if not (C > 0 and np.isfinite(C) and tol > 0 and np.isfinite(tol)) or max_iter < 0:
            raise ValueError('svm_fit: C and tol must be finite and > 0, max_iter >= 0')
        alpha = np.zeros(tr_off[-1]); rho = np.zeros(nj); n_iter = np.zeros(nj, np.int64); status = np.zeros(nj, np.int32)
        correct = np.zeros(nj, np.int64); dec = np.zeros(max(int(va_off[-1]), 1))
        prm = _lib.SvmParams(float(C), float(tol), int(max_iter))
        check(lib().mc_svm_fit(self._ctx, _lib.C.byref(prm), _ptr(X), _ptr(y), n, d, nj, _ptr(tr_off), _ptr(tr_idx), _ptr(va_off),
                               _ptr(va_idx), _ptr(g), _ptr(alpha), _ptr(rho), _ptr(n_iter), _ptr(status), _ptr(correct), _ptr(dec)))
        return [dict(alpha=alpha[tr_off[j]:tr_off[j + 1]].copy(), rho=float(rho[j]), n_iter=int(n_iter[j]), status=int(status[j]),
                     val_dec=dec[va_off[j]:va_off[j + 1]].copy(), val_correct=int(correct[j]), n_val=len(va[j])) for j in range(nj)]

    @_serialized
    def lr_fit(self, X, y, jobs, seeds, C=1.0, tol=1e-4, max_iter=100):
        """Fit one L1 logistic regression per job on the GPU (mc_lr_fit: every job a workgroup of k7_lr_fit, liblinear's
        solve_l1r_lr).  jobs: [(train_rows, validation_rows)] index arrays into X / y (y in {0, 1}, both classes in every job's
        training rows); seeds: a 31-bit liblinear seed per job.  -> per job a dict: coef [d] (toward class 1), intercept, n_iter
        (Newton iterations), status (1: max_iter was reached), val_dec, val_correct, n_val."""
        X, y, tr, va, tr_off, va_off, tr_idx, va_idx = self._fit_jobs(X, y, jobs, 'lr_fit')
        n, d = X.shape
        nj = len(jobs)
        sd = np.asarray(seeds, dtype=np.int64)
        if len(sd) != nj or (sd < 0).any() or (sd >= 2 ** 32).any():
            raise ValueError('lr_fit: one seed in 0 .. 2^32 - 1 per job is needed')
        if not (C > 0 and np.isfinite(C) and tol > 0 and np.isfinite(tol)) or not 1 <= max_iter <= 10 ** 6:
            raise ValueError('lr_fit: C and tol must be finite and > 0, max_iter in 1 .. 10^6')
        sd = np.ascontiguousarray(sd, dtype=np.uint32)
        coef = np.zeros((nj, d)); intercept = np.zeros(nj); n_iter = np.zeros(nj, np.int32); status = np.zeros(nj, np.int32)
        correct = np.zeros(nj, np.int64); dec = np.zeros(max(int(va_off[-1]), 1))
        prm = _lib.LrParams(float(C), float(tol), int(max_iter), 0)
        check(lib().mc_lr_fit(self._ctx, _lib.C.byref(prm), _ptr(X), _ptr(y), n, d, nj, _ptr(tr_off), _ptr(tr_idx), _ptr(va_off),
                              _ptr(va_idx), _ptr(sd), _ptr(coef), _ptr(intercept), _ptr(n_iter), _ptr(status), _ptr(correct), _ptr(dec)))
        return [dict(coef=coef[j].copy(), intercept=float(intercept[j]), n_iter=int(n_iter[j]), status=int(status[j]),
                     val_dec=dec[va_off[j]:va_off[j + 1]].copy(), val_correct=int(correct[j]), n_val=len(va[j])) for j in range(nj)]

    @_serialized
    def nb_fit(self, X, y, jobs, var_smoothing=1e-9):
        """Fit one Gaussian naive Bayes per job on the GPU (mc_nb_fit: every job a workgroup of k7_nb_fit, GaussianNB's fit).
        jobs as lr_fit's (both classes in every job's training rows, not all of them equal).  -> per job a dict: theta [2, d],
        var [2, d] (smoothing included), epsilon, class_count [2], val_correct, n_val."""
        X, y, tr, va, tr_off, va_off, tr_idx, va_idx = self._fit_jobs(X, y, jobs, 'nb_fit', need_spread=True)
        n, d = X.shape
        nj = len(jobs)
        if not (var_smoothing > 0 and np.isfinite(var_smoothing)):
            raise ValueError('nb_fit: var_smoothing must be finite and > 0')
        theta = np.zeros((nj, 2, d)); var = np.zeros((nj, 2, d)); eps = np.zeros(nj); count = np.zeros((nj, 2), np.int64)
        correct = np.zeros(nj, np.int64)
        prm = _lib.NbParams(float(var_smoothing))
        check(lib().mc_nb_fit(self._ctx, _lib.C.byref(prm), _ptr(X), _ptr(y), n, d, nj, _ptr(tr_off), _ptr(tr_idx), _ptr(va_off),
                              _ptr(va_idx), _ptr(theta), _ptr(var), _ptr(eps), _ptr(count), _ptr(correct)))
        return [dict(theta=theta[j].copy(), var=var[j].copy(), epsilon=float(eps[j]), class_count=count[j].copy(),
                     val_correct=int(correct[j]), n_val=len(va[j])) for j in range(nj)]

    @_serialized
    def svm_sigmoid_train(self, dec, y):
        """libsvm's sigmoid_train on the GPU: the Platt parameters (A, B) of decision values dec with labels y (0: libsvm's +1)."""
        dec = np.ascontiguousarray(dec, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        if dec.ndim != 1 or len(dec) < 1 or len(y) != len(dec) or not np.isfinite(dec).all() or (y > 1).any():
            raise ValueError('svm_sigmoid_train: finite decision values with a label in {0, 1} each are needed')
        A, B = C.c_double(), C.c_double()
        check(lib().mc_svm_sigmoid_train(self._ctx, _ptr(dec), _ptr(y), len(dec), C.byref(A), C.byref(B)))
        return A.value, B.value

    # ---- the per-site summary of a .diffs file (csrc/bed/mc_bedsum.hip) ----
    @_serialized
    def bed_summarise(self, path=None, text=None, min_depth=15, mod_threshold=0.5, control=False, with_probs=False, gff=False,
                      positions_path=None, positions_text=None, ref_path=None, ref_text=None, site_stats=False):
        """The bytes make_bed writes for a `.diffs.<k>` file (`path`) or its text (`text`, bytes), made on the GPU; with
        `positions_path` (beside `path`) or `positions_text` (beside `text`) what make_bed -p writes: the rows at the listed
        positions, every entry, two t-test columns in a BED row.
        With `ref_path` / `ref_text` (a FASTA: make_bed --ref) the GFF attributes carry the 41 bases around the site; with
        `site_stats` --gff --vo is made (fracLow, fracUp, identificationQv: mc_bed_params.site_stats) -- without it that combination
        declines, as it always did.
        -> (bytes, number of sites, None), or (None, 0, reason) when the device declines: the caller runs the host code."""
        if (path is None) == (text is None):
            raise ValueError('bed_summarise: a path or a text')
        if (positions_path is not None and path is None) or (positions_text is not None and text is None):
            raise ValueError('bed_summarise: positions_path goes with path, positions_text with text')
        if (ref_path is not None and path is None) or (ref_text is not None and text is None):
            raise ValueError('bed_summarise: ref_path goes with path, ref_text with text')
        d = int(min_depth)
        prm = _lib.BedParams(max(-2 ** 62, min(2 ** 62, d)), float(mod_threshold), int(bool(control)), int(bool(with_probs)), int(bool(gff)),
                             int(bool(site_stats) or ref_path is not None or ref_text is not None))
        out, n_out, n_sites, status = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32()
        (src, keep), (pos, keep_pos), (ref, keep_ref) = _source(path, text), _source(positions_path, positions_text), _source(ref_path, ref_text)
        check(lib().mc_bed_summarise(self._ctx, src, pos, ref, C.byref(prm), C.byref(out), C.byref(n_out), C.byref(n_sites), C.byref(status)))
        del keep, keep_pos, keep_ref
        if status.value != 0:
            return None, 0, last_error()
        return _blob(out.value, n_out.value), int(n_sites.value), None

    @_serialized
    def bed_last_stats(self):
        """Figures of the last bed_summarise: lines, counted rows, entries, sites, longest probe chain, the decline, milliseconds."""
        return self._last_stats(lib().mc_bed_last_stats, _lib.BedStats)

    @_serialized
    def bed_release(self):
        check(lib().mc_bed_release(self._ctx))

    # ---- the merge behind `-t N` (csrc/merge/mc_rowmerge.hip) ----
    @_serialized
    def merge_rows(self, paths=None, text=None, out_path=None):
        """`sort -n -k2 | uniq` as mCaller.merge_like_sort_uniq does it, on the GPU: over the part files `paths` into `out_path`
        (written beside it and renamed when complete; the part files stay), or over one `text` (bytes).
        -> (lines written, None) / (the merged bytes, None), or (None, reason) when the device declines: the caller runs the host code."""
        if (paths is None) == (text is None) or (paths is not None and out_path is None):
            raise ValueError('merge_rows: part files and an output path, or a text')
        status = C.c_int32()
        if paths is not None:
            arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
            n_lines = C.c_int64()
            check(lib().mc_rows_merge_files(self._ctx, arr, len(paths), os.fsencode(out_path), C.byref(n_lines), C.byref(status)))
            if status.value != 0:
                return None, last_error()
            return int(n_lines.value), None
        text = bytes(text)
        out, n_out = C.c_void_p(), C.c_int64()
        check(lib().mc_rows_merge_text(self._ctx, text, len(text), C.byref(out), C.byref(n_out), C.byref(status)))
        if status.value != 0:
            return None, last_error()
        return _blob(out.value, n_out.value), None

    @_serialized
    def merge_rows_last_stats(self):
        """Figures of the last merge_rows: bytes, lines in and out, rounds, radix passes, lines still tied after the numeric key,
        the largest group finished by comparison, the decline (line, reason, file), kernel bytes, milliseconds."""
        return self._last_stats(lib().mc_rows_merge_last_stats, _lib.RowsMergeStats)

    @_serialized
    def merge_rows_release(self):
        check(lib().mc_rows_merge_release(self._ctx))

    # ---- decimal text -> double (csrc/mc_decimal.h) and the rows of a --training_tsv file (csrc/train/mc_trainrows.hip) ----
    @_serialized
    def parse_doubles(self, tokens):
        """float() of every token (bytes) by mc_decimal.h's device build, a lane per token (mc_parse_doubles_device, tests).
        -> (float64 [n], 0.0 where declined; ok: bool [n])."""
        tokens = [bytes(t) for t in tokens]
        length = np.asarray([len(t) for t in tokens], dtype=np.int32)
        off = np.zeros(len(tokens), dtype=np.int64)
        if len(tokens) > 1:
            off[1:] = np.cumsum(length[:-1], dtype=np.int64)
        text = b''.join(tokens)
        out = np.zeros(len(tokens), dtype=np.float64)
        ok = np.zeros(len(tokens), dtype=np.uint8)
        check(lib().mc_parse_doubles_device(self._ctx, text, len(text), _ptr(off), _ptr(length), len(tokens), _ptr(out), _ptr(ok)))
        return out, ok.astype(bool)

    @_serialized
    def tstat(self, n, mean, var):
        """t and log10 p of one-sample t-tests from (rows, mean, sample variance) triples by mc_tstat.h's device build, a lane
        per triple (mc_tstat_device, tests) -> (status bits int32 [k], t float64 [k], log10 p float64 [k])."""
        n, mean, var = (np.ascontiguousarray(a, dtype=np.float64) for a in (n, mean, var))
        if not (n.ndim == 1 and n.shape == mean.shape == var.shape):
            raise ValueError('tstat: three arrays of one length')
        t, l, st = np.zeros(len(n)), np.zeros(len(n)), np.zeros(len(n), dtype=np.int32)
        check(lib().mc_tstat_device(self._ctx, _ptr(n), _ptr(mean), _ptr(var), len(n), _ptr(t), _ptr(l), _ptr(st)))
        return st, t, l

    @_serialized
    def hypergeom_tail(self, N, K, d, k):
        """P(X >= k) for X ~ Hypergeometric(N, K, d) and the derived bound on its error by mc_hypergeom.h's device build, a lane
        per case, one launch (mc_hypergeom_tail_device, tests and tools/hypergeom_error.py) -> (tail float64 [n], err float64 [n]);
        NaN where the arguments are out of range."""
        N, K, d, k = (np.ascontiguousarray(a, dtype=np.int64) for a in (N, K, d, k))
        if not (N.ndim == 1 and N.shape == K.shape == d.shape == k.shape):
            raise ValueError('hypergeom_tail: four arrays of one length')
        tail, err = np.zeros(len(N)), np.zeros(len(N))
        check(lib().mc_hypergeom_tail_device(self._ctx, _ptr(N), _ptr(K), _ptr(d), _ptr(k), len(N), _ptr(tail), _ptr(err)))
        return tail, err

    @_serialized
    def hypergeom_masses(self, N, K, d):
        """The bucket masses behind all 101 tails of X ~ Hypergeometric(N, K, d) and the derived bound on their summed error by
        mc_hypergeom.h's device build, a lane per case, one launch (mc_hypergeom_masses_device, tests and tools/hypergeom_error.py)
        -> (mass float64 [n, 102], err float64 [n]); NaN where the arguments are out of range."""
        N, K, d = (np.ascontiguousarray(a, dtype=np.int64) for a in (N, K, d))
        if not (N.ndim == 1 and N.shape == K.shape == d.shape):
            raise ValueError('hypergeom_masses: three arrays of one length')
        mass, err = np.zeros((len(N), _lib.ABI.constants['MC_HYPERGEOM_BUCKETS'])), np.zeros(len(N))
        check(lib().mc_hypergeom_masses_device(self._ctx, _ptr(N), _ptr(K), _ptr(d), len(N), _ptr(mass), _ptr(err)))
        return mass, err

    @_serialized
    def fisher_exact(self, K1, n1, K2, n2):
        """log10 of the two-sided p of Fisher's exact test on K1 of n1 against K2 of n2, its derived bound and the status bits
        (MC_FISHER_*) by mc_fisher.h's device build, a lane per table, one launch (mc_fisher_exact_device)
        -> (log10_p float64 [n], bound float64 [n], status int32 [n])."""
        K1, n1, K2, n2 = (np.ascontiguousarray(a, dtype=np.int64) for a in (K1, n1, K2, n2))
        if not (K1.ndim == 1 and K1.shape == n1.shape == K2.shape == n2.shape):
            raise ValueError('fisher_exact: four arrays of one length')
        l, b, st = np.zeros(len(K1)), np.zeros(len(K1)), np.zeros(len(K1), dtype=np.int32)
        check(lib().mc_fisher_exact_device(self._ctx, _ptr(K1), _ptr(n1), _ptr(K2), _ptr(n2), len(K1), _ptr(l), _ptr(b), _ptr(st)))
        return l, b, st

    @_serialized
    def bh_adjust(self, L, bound):
        """The Benjamini-Hochberg adjustment of one column of log10 p (NaN: an untested row) on the GPU: a device-wide radix sort of
        the rows' keys, the terms, a two-level minimum from the end (mc_bh_adjust_device; csrc/compare/mc_cmpfdr.inc)
        -> (Q float64 [n]: log10 q, rounded float64 [n]: np.round(0.0 - Q, 3), status: MC_BH_* bits)."""
        L, bound = np.ascontiguousarray(L, dtype=np.float64), np.ascontiguousarray(bound, dtype=np.float64)
        if not (L.ndim == 1 and L.shape == bound.shape):
            raise ValueError('bh_adjust: two arrays of one length')
        Q, rounded, st = np.zeros(len(L)), np.zeros(len(L)), C.c_int32()
        check(lib().mc_bh_adjust_device(self._ctx, _ptr(L), _ptr(bound), len(L), _ptr(Q), _ptr(rounded), C.byref(st)))
        return Q, rounded, int(st.value)

    @_serialized
    def gff_site_stats(self, arrays, frac):
        """fracLow, fracUp and 100 * mean of make_bed --gff --vo for every array of probabilities (frac: its entry's fraction) by
        mc_npsum.h's device build, a workgroup per array (mc_gff_site_stats_device, tests)
        -> (status bits int32 [k], float64 [k, 6]: fracLow, fracUp, 100 * mean, mean, var, se)."""
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
        frac = np.ascontiguousarray(frac, dtype=np.float64)
        if len(frac) != len(arrays) or any(a.ndim != 1 or len(a) < 1 for a in arrays):
            raise ValueError('gff_site_stats: a fraction for every array, no array empty')
        off = np.zeros(len(arrays) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(a) for a in arrays], dtype=np.int64)
        p = np.concatenate(arrays) if arrays else np.zeros(0)
        out, st = np.zeros((len(arrays), 6)), np.zeros(len(arrays), dtype=np.int32)
        check(lib().mc_gff_site_stats_device(self._ctx, _ptr(p), _ptr(off), _ptr(frac), len(arrays), _ptr(out), _ptr(st)))
        return st, out

    @_serialized
    def npsum_se(self, var, n):
        """sqrt(var) / sqrt(n) by mc_npsum.h's device build, a lane per pair (mc_npsum_se_device, tests)."""
        var, n = (np.ascontiguousarray(a, dtype=np.float64) for a in (var, n))
        if not (var.ndim == 1 and var.shape == n.shape):
            raise ValueError('npsum_se: two arrays of one length')
        se = np.zeros(len(var))
        check(lib().mc_npsum_se_device(self._ctx, _ptr(var), _ptr(n), len(var), _ptr(se)))
        return se

    @_serialized
    def training_rows(self, path=None, text=None, pairs=()):
        """The matrices of a `.diffs.<k>.train` file (`path`) or its text (`text`, bytes), made on the GPU; `pairs`: the
        two-character centre pairs a context may have.  -> (labels in first-occurrence order, {label: float64 [n, nf]},
        {label: 'S' array [n]} of the contexts, None) -- copies, the caller's own --, or (None, None, None, reason) when the device
        declines: the caller runs the host code."""
        if (path is None) == (text is None):
            raise ValueError('training_rows: a path or a text')
        pairs = [p.encode('ascii') if isinstance(p, str) else bytes(p) for p in pairs]
        if any(len(p) != 2 for p in pairs):
            raise ValueError('training_rows: a centre pair is two characters')
        blob = b''.join(pairs)
        view, status = _lib.TrainRowsView(), C.c_int32()
        src, keep = _source(path, text)
        check(lib().mc_train_rows(self._ctx, src, blob, len(pairs), C.byref(view), C.byref(status)))
        del keep
        if status.value != 0:
            return None, None, None, last_error()
        nf, width, total = view.n_features, view.ctx_width, view.n_rows_total
        X = np.empty((total, nf), dtype=np.float64)
        ctx = np.empty(total, dtype='S%d' % max(width, 1))
        if total:                                                 # (one copy each, out of the context's pinned memory)
            C.memmove(X.ctypes.data, view.X, X.nbytes)
            C.memmove(ctx.ctypes.data, view.contexts, ctx.nbytes)
        names = _blob(view.label_bytes, view.label_off[view.n_labels])
        labels, sig, grp, at = [], {}, {}, 0
        for i in range(view.n_labels):
            label = names[view.label_off[i]:view.label_off[i + 1]].decode('ascii')
            n = int(view.n_rows[i])
            labels.append(label)
            sig[label], grp[label] = X[at:at + n], ctx[at:at + n]
            at += n
        return labels, sig, grp, None

    @_serialized
    def training_rows_last_stats(self):
        """Figures of the last training_rows: lines, kept rows, labels, features, the decline, milliseconds."""
        return self._last_stats(lib().mc_train_rows_last_stats, _lib.TrainRowsStats)

    @_serialized
    def training_rows_release(self):
        check(lib().mc_train_rows_release(self._ctx))

    # ---- the evaluation file of a .diffs file against labelled positions (csrc/eval/mc_evalcalls.hip) ----
    @_serialized
    def eval_calls(self, path=None, text=None, positions_path=None, positions_text=None, min_depth=15, depths=(1, 2, 5, 10, 15, 20, 30, 50)):
        """The bytes evaluate.evaluate_calls gives for a `.diffs.<k>` file (`path`) or its text (`text`, bytes) against the labelled
        positions (`positions_path` or `positions_text`), made on the GPU -> (bytes, None), or (None, reason) when the device
        declines: the caller runs the host statement."""
        if (path is None) == (text is None) or (positions_path is None) == (positions_text is None):
            raise ValueError('eval_calls: a path or a text, and the positions as a path or a text')
        depths = [int(d) for d in depths]
        if len(depths) > 16:
            raise ValueError('eval_calls: at most 16 depths')
        prm = _lib.EvalParams()
        prm.min_depth, prm.n_depths = max(-2 ** 62, min(2 ** 62, int(min_depth))), len(depths)
        for i, d in enumerate(depths):
            prm.depths[i] = max(-1, min(2 ** 30, d))
        out, n_out, status = C.c_void_p(), C.c_int64(), C.c_int32()
        (src, keep), (pos, keep_pos) = _source(path, text), _source(positions_path, positions_text)
        check(lib().mc_eval_calls(self._ctx, src, pos, C.byref(prm), C.byref(out), C.byref(n_out), C.byref(status)))
        del keep, keep_pos
        if status.value != 0:
            return None, last_error()
        return _blob(out.value, n_out.value), None

    @_serialized
    def eval_calls_last_stats(self):
        """Figures of the last eval_calls: lines, kept / unlabelled / non-M rows, sites, (site, depth) pairs, the longest probe chain,
        the largest derived bound of a printed value, the decline (file, line, reason), milliseconds."""
        return self._last_stats(lib().mc_eval_last_stats, _lib.EvalStats)

    @_serialized
    def eval_calls_release(self):
        check(lib().mc_eval_release(self._ctx))

    # ---- the read qualities of a FASTQ file (csrc/fastq/mc_fastqual.hip) ----
    @_serialized
    def fastq_qualities(self, path=None, text=None):
        """One (key, mean phred) pair per record of a FASTQ file (`path`) or its text (`text`, bytes), made on the GPU
        -> (keys: list of str, means: float64 [n], None) -- copies, the caller's own --, or (None, None, reason) when the device
        declines: the caller runs the host reader."""
        if (path is None) == (text is None):
            raise ValueError('fastq_qualities: a path or a text')
        view, status = _lib.FastqQualityView(), C.c_int32()
        src, keep = _source(path, text)
        check(lib().mc_fastq_quality(self._ctx, src, C.byref(view), C.byref(status)))
        del keep
        if status.value != 0:
            return None, None, last_error()
        return _lib.fastq_unpack(view.key_pool, view.key_off, view.mean, int(view.n_records)) + (None,)

    @_serialized
    def fastq_qualities_last_stats(self):
        """Figures of the last fastq_qualities: bytes, lines, records, pieces and their size, the decline, milliseconds."""
        return self._last_stats(lib().mc_fastq_quality_last_stats, _lib.FastqQualityStats)

    @_serialized
    def fastq_qualities_release(self):
        check(lib().mc_fastq_quality_release(self._ctx))

    # ---- two --vo BED files compared per site (csrc/compare/mc_bedcompare.hip) ----
    @_serialized
    def bed_compare(self, path1=None, path2=None, text1=None, text2=None, contigs1=None, contigs2=None, fisher=False, fdr=False):
        """The rows of compare_genomes for two `make_bed --vo` files (`path1`, `path2`) or their texts (`text1`, `text2`, bytes),
        made on the GPU -> (blob: bytes, n_sites, None), or (None, 0, reason) when the device declines: the caller runs the
        host statement.  contigs1 / contigs2 (compare_genomes.read_fai's (names, lens, offs) of the two genomes): the comparison
        through the alignment map that xmfa_map left in the context; bed_compare_last_unaligned() then says how many lines of
        bed1 had no image.  fisher / fdr: the columns behind nlp_ks (compare_genomes --fisher --fdr; mc_bed_compare_with): Fisher's
        exact test on the two lines' counts, the Benjamini-Hochberg q-values of every -log10 p column."""
        if (path1 is None) != (path2 is None) or (text1 is None) != (text2 is None) or (path1 is None) == (text1 is None):
            raise ValueError('bed_compare: two paths or two texts')
        if (contigs1 is None) != (contigs2 is None):
            raise ValueError('bed_compare: the contigs of both genomes or of neither')
        out, n_out, n_sites, status = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32()
        self._unaligned = None
        n_unaligned = C.c_int64()
        (bed1, keep1), (bed2, keep2) = _source(path1, text1), _source(path2, text2)
        t1, t2, keep = None, None, None
        if contigs1 is not None:
            (t1, keep_t1), (t2, keep_t2) = _contig_table(contigs1), _contig_table(contigs2)
            t1, t2, keep = C.byref(t1), C.byref(t2), (keep_t1, keep_t2)
        if fisher or fdr:
            opt = _lib.ABI.structs['mc_cmp_options'](int(bool(fisher)), int(bool(fdr)))
            check(lib().mc_bed_compare_with(self._ctx, bed1, bed2, t1, t2, C.byref(opt), C.byref(out), C.byref(n_out), C.byref(n_sites),
                                            C.byref(n_unaligned), C.byref(status)))
        else:
            check(lib().mc_bed_compare(self._ctx, bed1, bed2, t1, t2, C.byref(out), C.byref(n_out), C.byref(n_sites), C.byref(n_unaligned),
                                       C.byref(status)))
        del keep, keep1, keep2
        if contigs1 is not None and status.value == 0:
            self._unaligned = int(n_unaligned.value)
        if status.value != 0:
            return None, 0, last_error()
        return _blob(out.value, n_out.value), int(n_sites.value), None

    def bed_compare_last_unaligned(self):
        """bed1's lines without an image in the last bed_compare through an alignment (None: it declined, or had none)."""
        return getattr(self, '_unaligned', None)

    # ---- a native sample against a control, site by site (csrc/compare/mc_sitegroup.inc groups the lines, mc_curcompare.inc) ----
    @_serialized
    def currents_compare(self, path1=None, path2=None, text1=None, text2=None, depth=15, fdr=False, by=None, threshold=2.0):
        """The rows of compare_currents for the .diffs files of a native sample and a control (`path1`, `path2`) or their texts
        (`text1`, `text2`, bytes), made on the GPU -> (blob: bytes, bed: bytes, n_sites, n_sig, None), or (None, None, 0, 0, reason)
        when the device declines: the caller runs the host statement.  by ('mwu', 'rs', 't', 'ks'; None: no bed): the rows whose
        printed value of that test (fdr: its q-value) is at least `threshold` are the bed's lines."""
        if (path1 is None) != (path2 is None) or (text1 is None) != (text2 is None) or (path1 is None) == (text1 is None):
            raise ValueError('currents_compare: two paths or two texts')
        tests = ('mwu', 'rs', 't', 'ks')
        if by is not None and by not in tests:
            raise ValueError('currents_compare: by is one of mwu, rs, t, ks')
        if int(depth) < 2:
            raise ValueError('currents_compare: a depth of at least 2')
        # c and log10(c) from the native text's first row: the constant is NumPy's, the bits the host statement adds
        c = _first_row_columns(path1, text1)
        opt = _lib.CurOptions(int(depth), int(bool(fdr)), -1 if by is None else tests.index(by), min(c, 65535), float(threshold),
                              float(np.log10(c)) if c >= 1 else 0.0)
        res, status = _lib.CurResult(), C.c_int32()
        (src1, keep1), (src2, keep2) = _source(path1, text1), _source(path2, text2)
        check(lib().mc_currents_compare(self._ctx, src1, src2, C.byref(opt), C.byref(res), C.byref(status)))
        del keep1, keep2
        if status.value != 0:
            return None, None, 0, 0, last_error()
        return _blob(res.out, res.n_out), _blob(res.bed, res.n_bed), int(res.n_sites), int(res.n_sig), None

    @_serialized
    def currents_compare_last_stats(self):
        """Figures of the last currents_compare: bytes, lines, keys, kept sites, the rank kernels' shares, the decline, milliseconds."""
        return self._last_stats(lib().mc_currents_compare_last_stats, _lib.CurStats)

    @_serialized
    def currents_compare_release(self):
        check(lib().mc_currents_compare_release(self._ctx))

    # ---- the rows of every site split in two by their currents (csrc/compare/mc_sitegroup.inc groups the lines, mc_sitecluster.inc) ----
    @_serialized
    def sites_cluster(self, path=None, text=None, depth=15, max_depth=256, metric='correlation', mixed=False, min_minor=0.2, min_gap=2.0):
        """The rows of cluster_sites for a .diffs file (`path`) or its text (`text`, bytes), made on the GPU -> (blob: bytes, bed:
        bytes, n_sites, n_mixed, None), or (None, None, 0, 0, reason) when the device declines: the caller runs the host statement.
        mixed: the rows whose smaller cluster holds at least `min_minor` of the rows and whose h_top is at least `min_gap` times
        h_sub are the bed's lines."""
        if (path is None) == (text is None):
            raise ValueError('sites_cluster: a path or a text')
        if metric not in _lib.CLU_METRIC:
            raise ValueError('sites_cluster: metric is correlation or euclidean')
        if int(depth) < 2 or not 2 <= int(max_depth) <= _lib.CLU_MAX_DEPTH:
            raise ValueError('sites_cluster: a depth of at least 2 and a max_depth of 2 to %d' % _lib.CLU_MAX_DEPTH)
        c = _first_row_columns(path, text)
        opt = _lib.CluOptions(int(depth), int(max_depth), _lib.CLU_METRIC[metric], int(bool(mixed)), min(c, 65535), 0, float(min_minor),
                              float(min_gap))
        res, status = _lib.CluResult(), C.c_int32()
        src, keep = _source(path, text)
        check(lib().mc_sites_cluster(self._ctx, src, C.byref(opt), C.byref(res), C.byref(status)))
        del keep
        if status.value != 0:
            return None, None, 0, 0, last_error()
        return _blob(res.out, res.n_out), _blob(res.bed, res.n_bed), int(res.n_sites), int(res.n_mixed), None

    @_serialized
    def sites_cluster_last_stats(self):
        """Figures of the last sites_cluster: bytes, lines, keys, candidates, kept sites, the link kernels' shares, the slabs, the
        decline, milliseconds."""
        return self._last_stats(lib().mc_sites_cluster_last_stats, _lib.CluStats)

    @_serialized
    def sites_cluster_release(self):
        check(lib().mc_sites_cluster_release(self._ctx))

    # ---- methylation linkage between sites along reads (csrc/compare/mc_sitegroup.inc groups the lines, mc_readphase.inc) ----
    @_serialized
    def reads_phase(self, path=None, text=None, depth=15, max_dist=1000, min_reads=10, min_margin=2, fdr=False, threshold=None):
        """The rows of phase_reads for a .diffs file (`path`) or its text (`text`, bytes), made on the GPU -> (blob: bytes, reads:
        bytes, bed: bytes, n_pairs, n_reads, n_linked, None), or (None, None, None, 0, 0, 0, reason) when the device declines: the
        caller runs the host statement.  threshold (None: no bed): the kept sites of a written pair whose printed -log10 p (fdr:
        q) is at least it are the bed's lines."""
        if (path is None) == (text is None):
            raise ValueError('reads_phase: a path or a text')
        if min(int(depth), int(max_dist), int(min_reads), int(min_margin)) < 1:
            raise ValueError('reads_phase: depth, max_dist, min_reads and min_margin of at least 1')
        if threshold is not None and float(threshold) != float(threshold):
            raise ValueError('reads_phase: a threshold that is a number')
        c = _first_row_columns(path, text)
        opt = _lib.PhaseOptions(int(depth), min(int(max_dist), 2 ** 31 - 1), min(int(min_reads), 2 ** 31 - 1), min(int(min_margin), 2 ** 31 - 1),
                                int(bool(fdr)), int(threshold is not None), min(c, 65535), 0, 0.0 if threshold is None else float(threshold))
        res, status = _lib.PhaseResult(), C.c_int32()
        src, keep = _source(path, text)
        check(lib().mc_reads_phase(self._ctx, src, C.byref(opt), C.byref(res), C.byref(status)))
        del keep
        if status.value != 0:
            return None, None, None, 0, 0, 0, last_error()
        return (_blob(res.out, res.n_out), _blob(res.reads, res.n_reads_bytes), _blob(res.bed, res.n_bed), int(res.n_pairs), int(res.n_reads),
                int(res.n_linked), None)

    @_serialized
    def reads_phase_last_stats(self):
        """Figures of the last reads_phase: bytes, lines, keys, kept sites, reads and who ordered them, the window, the counters, the
        pair instances, the three outputs, the decline, milliseconds."""
        return self._last_stats(lib().mc_reads_phase_last_stats, _lib.PhaseStats)

    @_serialized
    def reads_phase_release(self):
        check(lib().mc_reads_phase_release(self._ctx))

    # ---- the coordinate map of a Mauve alignment (csrc/compare/mc_xmfamap.inc) ----
    @_serialized
    def xmfa_map(self, path=None, text=None, n1=0, seqs=(1, 2), n2=None, view=True):
        """The map of an XMFA file (`path`, or its `text`, bytes) from genome seqs[0] (n1 bases) onto genome seqs[1] (n2 bases;
        None: 2^31 - 2, no END is beyond it), built on the GPU and kept in the context for bed_compare(contigs1=, contigs2=)
        -> (g2: int64 [n1 + 1], flip: uint8 [n1 + 1], None) -- copies; (None, None, None) with view=False --, or (None, None,
        reason) when the device declines: no map is kept, compare_genomes' host statement words the error."""
        if (path is None) == (text is None):
            raise ValueError('xmfa_map: a path or a text')
        v, status = _lib.XmfaMapView(), C.c_int32()
        pv = C.byref(v) if view else None
        n2 = (1 << 31) - 2 if n2 is None else int(n2)
        src, keep = _source(path, text)
        check(lib().mc_xmfa_map(self._ctx, src, int(seqs[0]), int(seqs[1]), int(n1), n2, pv, C.byref(status)))
        del keep
        if status.value != 0:
            return None, None, last_error()
        if not view:
            return None, None, None
        n = int(v.n1) + 1
        return (np.ctypeslib.as_array(C.cast(v.g2, C.POINTER(C.c_int64)), shape=(n,)).copy(),
                np.ctypeslib.as_array(C.cast(v.flip, C.POINTER(C.c_uint8)), shape=(n,)).copy(), None)

    @_serialized
    def xmfa_map_last_stats(self):
        """Figures of the last xmfa_map: bytes, lines, entries, blocks, paired blocks, columns, mapped bases, the decline,
        milliseconds."""
        return self._last_stats(lib().mc_xmfa_map_last_stats, _lib.XmfaStats)

    @_serialized
    def xmfa_map_release(self):
        check(lib().mc_xmfa_map_release(self._ctx))

    @_serialized
    def bed_compare_last_stats(self):
        """Figures of the last bed_compare: bytes, lines, keys, shared sites, the rank kernels' shares, the decline, milliseconds."""
        return self._last_stats(lib().mc_bed_compare_last_stats, _lib.CmpStats)

    @_serialized
    def bed_compare_release(self):
        check(lib().mc_bed_compare_release(self._ctx))

    # ---- methylated motifs from called sites (csrc/motifs/mc_motifscan.hip) ----
    @_serialized
    def motif_report(self, ref, path=None, control_path=None, text=None, control_text=None, base='A', shapes=('XXXX',), min_sites=20,
                     min_fraction=0.5, keep_all=False, iupac=False, iterative=False, max_motifs=16, left=False):
        """The rows of find_motifs for the reference `ref` ({id: upper-cased sequence}), the sites of a make_bed summary (`path`,
        or its `text`, bytes) and optionally a make_bed --control summary (`control_path` / `control_text`), made on the GPU ->
        (blob: bytes, n_rows, None), or (None, 0, reason) when the device declines: the caller runs the host statement.
        iupac: the rows merged into degenerate motifs (find_motifs --iupac).
        iterative: the first row of every round, at most max_motifs (find_motifs --iterative) -> a fourth value: with `left` the
        bytes of the --unexplained file, else None."""
        if iterative and not 1 <= int(max_motifs) <= 64:
            raise ValueError('motif_report: max_motifs is 1 to 64')
        if (path is None) == (text is None) or (path is None and control_path is not None) or (text is None and control_text is not None):
            raise ValueError('motif_report: paths or texts')
        ids = [name.encode('latin-1', 'replace') for name in ref]
        seqs = [seq.encode('latin-1', 'replace') for seq in ref.values()]
        lens = np.asarray([len(s) for s in seqs], dtype=np.int64).reshape(-1)
        seq_off = np.zeros(len(seqs) + 1, dtype=np.int64)
        seq_off[1:] = np.cumsum(lens, dtype=np.int64)
        seq = np.frombuffer(b''.join(seqs) + b'\0', dtype=np.uint8)
        id_off = np.zeros(len(ids) + 1, dtype=np.int64)
        id_off[1:] = np.cumsum([len(i) for i in ids], dtype=np.int64)
        id_pool = np.frombuffer(b''.join(ids) + b'\0', dtype=np.uint8)
        v = _lib.RefView()
        v.n_contigs = len(seqs)
        v.contig_len, v.seq_off, v.seq = _ptr(lens), _ptr(seq_off), _ptr(seq)
        v.n_seq_bytes = int(seq_off[-1])
        shapes = list(shapes)
        if not 1 <= len(shapes) <= 64 or any(len(s) > 24 for s in shapes):
            raise ValueError('motif_report: 1 to 64 shapes of at most 24 characters')
        P = _lib.MotifParams()
        P.base, P.n_shapes = ord(base), len(shapes)
        for i, s in enumerate(shapes):
            P.shapes[i].value = s.encode('ascii')
        P.min_sites, P.min_fraction, P.keep_all = int(min_sites), float(min_fraction), int(bool(keep_all))
        P.contig_ids, P.contig_id_off = _ptr(id_pool), _ptr(id_off)
        out, n_out, n_rows, status = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int32()
        (bed, keep), (control, keep_control) = _source(path, text), _source(control_path, control_text)
        check(lib().mc_motif_report(self._ctx, C.byref(v), bed, control, C.byref(P), int(bool(iupac)), int(max_motifs) if iterative else 0,
                                    C.byref(out), C.byref(n_out), C.byref(n_rows), C.byref(status)))
        del keep, keep_control
        blob = _blob(out.value, n_out.value) if status.value == 0 else b''
        if iterative:
            if status.value != 0:
                return None, 0, last_error(), None
            return blob, int(n_rows.value), None, (self._motif_left(list(ref), lens) if left else None)
        if status.value != 0:
            return None, 0, last_error()
        return blob, int(n_rows.value), None

    def _motif_left(self, names, lens):
        """The --unexplained file of the last motif_report(iterative=True): the two planes of left-over sites as bed lines, contigs
        in the reference's order, start ascending."""
        plus, minus, starts = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n_words, n_contigs = C.c_int64(), C.c_int32()
        check(lib().mc_motif_report_iter_left(self._ctx, C.byref(plus), C.byref(minus), C.byref(n_words), C.byref(starts), C.byref(n_contigs)))
        if n_words.value == 0 or n_contigs.value != len(names):
            raise RuntimeError('motif_report: the left-over sites of the last call are not there')
        bits = [np.unpackbits(np.frombuffer(C.string_at(p.value, n_words.value * 8), dtype=np.uint8), bitorder='little') for p in (plus, minus)]
        at = np.frombuffer(C.string_at(starts.value, len(names) * 8), dtype=np.int64) if names else ()
        out = []
        for name, n, g in zip(names, lens.tolist(), at):
            on = [b[g:g + n] for b in bits]
            for p in np.nonzero(on[0] | on[1])[0].tolist():
                out.append('%s\t%d\t%d\t.\t.\t%s\n' % (name, p, p + 1, '-' if on[1][p] else '+'))
        return ''.join(out).encode('latin-1', 'replace')

    @_serialized
    def motif_report_iter_last_stats(self):
        """Figures of the last motif_report(iterative=True): the rounds, the candidates every row explained, the methylated candidates
        left, the bytes counted against device memory, the decline, the milliseconds of the first and of all later rounds."""
        st = self._last_stats(lib().mc_motif_report_iter_last_stats, _lib.MotifIterStats)
        st['n_explained'] = list(st['n_explained'])[:st['n_rounds']]
        return st

    @_serialized
    def motif_report_last_stats(self):
        """Figures of the last motif_report: bytes, lines, candidates and sites, selected entries and rows, the stretch and the tables'
        placements, the decline, milliseconds."""
        return self._last_stats(lib().mc_motif_report_last_stats, _lib.MotifStats)

    @_serialized
    def motif_report_iupac_last_stats(self):
        """Figures of the last motif_report(iupac=True): good entries, pure and maximal patterns, the lattices' bytes, the decline."""
        return self._last_stats(lib().mc_motif_report_iupac_last_stats, _lib.MotifIupacStats)

    @_serialized
    def motif_report_release(self):
        check(lib().mc_motif_report_release(self._ctx))

    # ---- motif methylation per bin and the bins' nearest bins (csrc/motifs/mc_motifprofile.inc) ----
    @_serialized
    def motif_profile(self, ref, path=None, control_path=None, text=None, control_text=None, base='A', specs=(), window=0, min_sites=5,
                      neighbours=None, min_shared=2):
        """The two files of motif_profile for the reference `ref` ({id: upper-cased sequence}), the sites of a make_bed summary (`path`,
        or its `text`, bytes), optionally a make_bed --control summary, and `specs` (motif_profile.parse_profile_motifs), made on the
        GPU -> (profile: bytes, n_rows, neighbours: bytes, n_nn_rows, None), or (None, 0, None, 0, reason) when the device declines:
        the caller runs the host statement.  neighbours None: no second file (b'')."""
        if (path is None) == (text is None) or (path is None and control_path is not None) or (text is None and control_text is not None):
            raise ValueError('motif_profile: paths or texts')
        specs = list(specs)
        if not 1 <= len(specs) <= 64 or any(len(s.entries) != 1 for s in specs):
            raise ValueError('motif_profile: 1 to 64 motifs of one entry each')
        ids = [name.encode('latin-1', 'replace') for name in ref]
        seqs = [seq.encode('latin-1', 'replace') for seq in ref.values()]
        lens = np.asarray([len(s) for s in seqs], dtype=np.int64).reshape(-1)
        seq_off = np.zeros(len(seqs) + 1, dtype=np.int64)
        seq_off[1:] = np.cumsum(lens, dtype=np.int64)
        seq = np.frombuffer(b''.join(seqs) + b'\0', dtype=np.uint8)

        def pooled(items):
            off = np.zeros(len(items) + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(i) for i in items], dtype=np.int64)
            return np.frombuffer(b''.join(items) + b'\0', dtype=np.uint8), off
        id_pool, id_off = pooled(ids)
        letter_pool, letter_off = pooled([s.entries[0][0].encode('ascii') for s in specs])
        spec_pool, spec_off = pooled([s.text.encode('ascii') for s in specs])
        called = np.asarray([sum(1 << (i - 1) for i in s.entries[0][1]) for s in specs], dtype=np.uint32).reshape(-1)
        v = _lib.RefView()
        v.n_contigs = len(seqs)
        v.contig_len, v.seq_off, v.seq = _ptr(lens), _ptr(seq_off), _ptr(seq)
        v.n_seq_bytes = int(seq_off[-1])
        P = _lib.MotifProfileParams()
        P.base, P.n_motifs = ord(base), len(specs)
        P.letters, P.letters_off, P.called = _ptr(letter_pool), _ptr(letter_off), _ptr(called)
        P.specs, P.spec_off = _ptr(spec_pool), _ptr(spec_off)
        P.window, P.min_sites = int(window), int(min_sites)
        P.neighbours, P.min_shared = (0 if neighbours is None else int(neighbours)), int(min_shared)
        P.contig_ids, P.contig_id_off = _ptr(id_pool), _ptr(id_off)
        res, status = _lib.MotifProfileResult(), C.c_int32()
        (bed, keep), (control, keep_control) = _source(path, text), _source(control_path, control_text)
        check(lib().mc_motif_profile(self._ctx, C.byref(v), bed, control, C.byref(P), C.byref(res), C.byref(status)))
        del keep, keep_control
        if status.value != 0:
            return None, 0, None, 0, last_error()
        return _blob(res.out, res.n_out), int(res.n_rows), _blob(res.nn, res.n_nn), int(res.n_nn_rows), None

    @_serialized
    def motif_profile_last_stats(self):
        """Figures of the last motif_profile: bytes, lines, candidates and sites, bins, rows, defined bins, pairs, neighbour rows, the
        outputs' bytes, the decline, milliseconds."""
        return self._last_stats(lib().mc_motif_profile_last_stats, _lib.MotifProfileStats)

    @_serialized
    def motif_profile_release(self):
        check(lib().mc_motif_profile_release(self._ctx))

    @_serialized
    def twosample(self, xs, ys):
        """The nine values of a compare_genomes row for every pair of samples by mc_twosample.h's device build, a wave or a
        workgroup per pair (mc_twosample_device, tests) -> (status bits int32 [k], float64 [k, 9], float64 [k, 9] bounds)."""
        xs = [np.ascontiguousarray(a, dtype=np.float64) for a in xs]
        ys = [np.ascontiguousarray(a, dtype=np.float64) for a in ys]
        if len(xs) != len(ys) or any(a.ndim != 1 for a in xs + ys):
            raise ValueError('twosample: a y for every x')
        k = len(xs)
        x_off, y_off = np.zeros(k + 1, dtype=np.int64), np.zeros(k + 1, dtype=np.int64)
        x_off[1:] = np.cumsum([len(a) for a in xs], dtype=np.int64)
        y_off[1:] = np.cumsum([len(a) for a in ys], dtype=np.int64)
        x = np.concatenate(xs + [np.zeros(1)])
        y = np.concatenate(ys + [np.zeros(1)])
        out, bound, st = np.zeros((k, 9)), np.zeros((k, 9)), np.zeros(k, dtype=np.int32)
        check(lib().mc_twosample_device(self._ctx, _ptr(x), _ptr(x_off), _ptr(y), _ptr(y_off), k, _ptr(out), _ptr(bound), _ptr(st)))
        return st, out, bound

    @_serialized
    def mlp_forward(self, X, submodel):
        if getattr(self, '_clf', 'mlp') != 'mlp':
            return self.classifier_forward(X, submodel)
        X = np.ascontiguousarray(X, dtype=np.float64)
        sm = np.ascontiguousarray(submodel, dtype=np.uint8)
        p = np.empty(len(X), dtype=np.float64)
        check(lib().mc_mlp_forward(self._ctx, _ptr(X), _ptr(sm), len(X), _ptr(p)))
        return p


def forest_arrays(forests):
    """Concatenate the sub-models' trees into the flat arrays of mc_ctx_set_forest."""
    model_tree_off, tree_node_off = [0], [0]
    left, right, feature, threshold, value = [], [], [], [], []
    for f in forests:
        base = tree_node_off[-1]
        left.append(np.where(f.left >= 0, f.left + base, -1))
        right.append(np.where(f.right >= 0, f.right + base, -1))
        feature.append(f.feature)
        threshold.append(f.threshold)
        value.append(f.value)
        tree_node_off.extend((f.tree_off[1:] + base).tolist())
        model_tree_off.append(model_tree_off[-1] + f.n_trees)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dtype=dt)
    return dict(model_tree_off=np.asarray(model_tree_off, dtype=np.int32), tree_node_off=np.asarray(tree_node_off, dtype=np.int32),
                left=cat(left, np.int32), right=cat(right, np.int32), feature=cat(feature, np.int32),
                threshold=cat(threshold, np.float64), value=cat([v.reshape(-1) for v in value], np.float64))


_devices = {}


def get_device(index=None):
    index = default_device_index() if index is None else int(index)
    if index not in _devices:
        _devices[index] = Device(index)
    return _devices[index]
