"""ctypes binding of libmcaller_hip.so (C ABI: include/mcaller_hip.h).

The library holds the native eventalign parser and the HIP kernels.  There is no fallback: if the
shared object is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MCALLER_LIB') or os.path.join(_HERE, 'libmcaller_hip.so')      # (MCALLER_LIB: a variant build, tools/variants.sh)

ABI = _abi.load()      # include/mcaller_hip.h: the one statement of the structs, the constants and the prototypes
_K, _S = ABI.constants, ABI.structs

MC_MAX_K = _K['MC_MAX_K']
F_KMER_EQ, F_MODEL_N, F_SEG_START, F_NAME_START = (_K['MC_F_' + n] for n in ('KMER_EQ', 'MODEL_N', 'SEG_START', 'NAME_START'))
I_EMPTY_MASK, I_REV, I_TOO_MANY, I_MULTI, I_EDGE, I_NEXT_SHIFT = (
    _K['MC_I_' + n] for n in ('EMPTY_MASK', 'REV', 'TOO_MANY', 'MULTI', 'EDGE', 'NEXT_SHIFT'))
E_NO_FREE_SLOT = _K['MC_E_NO_FREE_SLOT']


class McError(RuntimeError):
    """An error of the library; `code`: what the call returned."""
    code = None


TableView = _S['mc_table_view']
RefView = _S['mc_ref_view']
IupacMotif = _S['mc_iupac_motif']
IupacSpec = _S['mc_iupac_spec']
DevParseResult = _S['mc_devparse_result']
CallsView = _S['mc_calls_view']
FormatArgs = _S['mc_format_args']
FitParams = _S['mc_fit_params']
ForestParams = _S['mc_forest_params']
ForestFitStats = _S['mc_forest_fit_stats']
SvmParams = _S['mc_svm_params']
LrParams = _S['mc_lr_params']
NbParams = _S['mc_nb_params']
TextSource = _S['mc_text_source']
BedParams = _S['mc_bed_params']
BedStats = _S['mc_bed_stats']
TrainRowsView = _S['mc_train_rows_view']
TrainRowsView.MAX_LABELS = _K['MC_TRAINROWS_MAX_LABELS']
TrainRowsStats = _S['mc_train_rows_stats']
RowsMergeStats = _S['mc_rows_merge_stats']
FastqQualityView = _S['mc_fastq_quality_view']
FastqQualityStats = _S['mc_fastq_quality_stats']
CmpStats = _S['mc_cmp_stats']
CurOptions = _S['mc_cur_options']
CurResult = _S['mc_cur_result']
CurStats = _S['mc_cur_stats']
CluOptions = _S['mc_clu_options']
CluResult = _S['mc_clu_result']
CluStats = _S['mc_clu_stats']
PhaseOptions = _S['mc_phase_options']
PhaseResult = _S['mc_phase_result']
PhaseStats = _S['mc_phase_stats']
ContigTable = _S['mc_contig_table']
XmfaMapView = _S['mc_xmfa_map_view']
XmfaStats = _S['mc_xmfa_stats']
MotifParams = _S['mc_motif_params']
MotifStats = _S['mc_motif_stats']
MotifIupacStats = _S['mc_motif_iupac_stats']
MotifIterStats = _S['mc_motif_iter_stats']
MotifProfileParams = _S['mc_motif_profile_params']
MotifProfileResult = _S['mc_motif_profile_result']
MotifProfileStats = _S['mc_motif_profile_stats']
EvalParams = _S['mc_eval_params']
EvalStats = _S['mc_eval_stats']
Params = _S['mc_params']

EVAL_DECLINE = ABI.prefixed('MC_EVAL_DECLINE_')
MOTIF_DECLINE = ABI.prefixed('MC_MOTIF_DECLINE_')
CMP_DECLINE = ABI.prefixed('MC_CMP_DECLINE_')
FASTQ_DECLINE = ABI.prefixed('MC_FASTQ_DECLINE_')
MERGE_DECLINE = ABI.prefixed('MC_MERGE_DECLINE_')
TW_STATUS = {'bad_n': 1, 'zero_var': 2, 'far_tail': 4, 'no_convergence': 8, 'all_equal': 16, 'tie': 32, 'unprintable': 64,
             'deep': 128}                                                                        # TW_* (csrc/mc_twosample.h)
CLU_METRIC = {'correlation': _K['MC_CLU_CORRELATION'], 'euclidean': _K['MC_CLU_EUCLIDEAN']}
CLU_WAVE_ROWS, CLU_LDS_ROWS, CLU_MAX_DEPTH = _K['MC_CLU_WAVE_ROWS'], _K['MC_CLU_LDS_ROWS'], _K['MC_CLU_MAX_DEPTH']
PHASE_WAVE_ROWS, PHASE_GROUP_ROWS, PHASE_MAX_DEPTH = _K['MC_PHASE_WAVE_ROWS'], _K['MC_PHASE_GROUP_ROWS'], _K['MC_PHASE_MAX_DEPTH']
CC_STATUS = {'nan': 1, 'range': 2, 'tie': 4, 'unprintable': 8}                                 # CC_* (csrc/mc_curcombine.h)
TW_NAMES = ('U', 'z_mwu', 'z_rs', 't', 'D', 'nlp_mwu', 'nlp_rs', 'nlp_t', 'nlp_ks')

_lib = None


def lib():
    """Load libmcaller_hip.so (once), every function typed as the header declares it.  Raises ImportError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError('%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                              '(hipcc --offload-arch=gfx950); there is no CPU fallback' % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        ABI.declare(L)
        _lib = L
    return _lib


def last_error():
    """The calling thread's last error text: why a call failed, or why it declined."""
    return lib().mc_last_error().decode('utf-8', 'replace')


def check(rc):
    if rc != 0:
        e = McError(last_error() or 'libmcaller_hip error %d' % rc)
        e.code = rc
        raise e


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_model_n(flags):
    """The model-N bit column of a flag column (mc_pack_model_n): bit r & 7 of byte r >> 3 is (flags[r] & F_MODEL_N) != 0."""
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    out = np.zeros((len(flags) + 7) // 8, dtype=np.uint8)
    if len(flags):
        lib().mc_pack_model_n(_ptr(flags), len(flags), _ptr(out))
    return out


def pack_idx_rel(event_idx):
    """The index-relation column of an event-index column (mc_pack_idx_rel): a uint16 per eight rows, bit e of word u is
    event_idx[8u + e] > event_idx[8u + e - 1], bit 8 + e is `<` (row 0 and the bits beyond the last row: 0)."""
    event_idx = np.ascontiguousarray(event_idx, dtype=np.int32)
    out = np.zeros((len(event_idx) + 7) // 8, dtype=np.uint16)
    if len(event_idx):
        lib().mc_pack_idx_rel(_ptr(event_idx), len(event_idx), _ptr(out))
    return out


def _from_ptr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n)


class PinnedArray(object):
    """A numpy array over a block of the library's pinned host pool (mc_host_alloc); the block goes back to the pool
    when the object dies."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib().mc_host_alloc(max(n, 1) + 64)
        if not self.ptr:
            raise MemoryError('mc_host_alloc(%d)' % n)
        buf = (C.c_char * max(n, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def __del__(self):
        try:
            if self.ptr:
                lib().mc_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class Table(object):
    """Columnar event table on the host: numpy arrays + a TableView over them.  The event and model currents are one
    column of (event, model) pairs, `evmu` [n, 2]; `event_e4` / `model_e4` are its two halves (strided views)."""

    def __init__(self, pos, event_e4, model_e4, event_idx, flags, seg_row_begin, seg_read, seg_contig, n_reads,
                 read_names=None, unknown=(), owner=None, evmu=None, model_n_bits=None, idx_rel_bits=None):
        self.pos = np.ascontiguousarray(pos, dtype=np.int32)
        if evmu is None:
            evmu = np.empty((len(self.pos), 2), dtype=np.int32)
            evmu[:, 0] = event_e4
            evmu[:, 1] = model_e4
        self.evmu = np.ascontiguousarray(evmu, dtype=np.int32).reshape(-1, 2)
        self.event_idx = np.ascontiguousarray(event_idx, dtype=np.int32)
        self.flags = np.ascontiguousarray(flags, dtype=np.uint8)
        # the model-N bit column the table's maker wrote with the flags (a parser, pinned()); None: bare arrays
        self._model_n_bits = None if model_n_bits is None else np.ascontiguousarray(model_n_bits, dtype=np.uint8)
        # ... and the index-relation column written with the event indices; None: bare arrays
        self._idx_rel_bits = None if idx_rel_bits is None else np.ascontiguousarray(idx_rel_bits, dtype=np.uint16)
        self.seg_row_begin = np.ascontiguousarray(seg_row_begin, dtype=np.int64)
        self.seg_read = np.ascontiguousarray(seg_read, dtype=np.int32)
        self.seg_contig = np.ascontiguousarray(seg_contig, dtype=np.int32)
        self.n_reads = int(n_reads)
        self.read_names = read_names
        self.unknown = list(unknown)
        self._owner = owner
        self.n_rows = len(self.pos)
        self.n_seg = len(self.seg_read)

    @property
    def event_e4(self):
        return self.evmu[:, 0]

    @property
    def model_e4(self):
        return self.evmu[:, 1]

    @property
    def model_n_bits(self):
        """The model-N bit column (mc_table_view.model_n_bits): the maker's, or -- a table built from bare arrays, whose flags
        may have been edited since -- packed from the flags as they are now (mc_pack_model_n)."""
        if self._model_n_bits is not None:
            return self._model_n_bits
        return None if self.flags is None else pack_model_n(self.flags)

    @property
    def idx_rel_bits(self):
        """The index-relation column (mc_table_view.idx_rel_bits): the maker's, or -- a table built from bare arrays, whose
        indices may have been edited since -- packed from the event indices as they are now (mc_pack_idx_rel)."""
        if self._idx_rel_bits is not None:
            return self._idx_rel_bits
        return None if self.event_idx is None else pack_idx_rel(self.event_idx)

    def pinned(self):
        """A copy whose columns sit in the pinned host pool (what mc_ctx_upload_table_async wants to read from)."""
        keep = []

        def pin(a):
            h = PinnedArray(a.shape, a.dtype)
            h.array[...] = a
            keep.append(h)
            return h.array
        t = Table(pin(self.pos), None, None, pin(self.event_idx), pin(self.flags), self.seg_row_begin, self.seg_read,
                  self.seg_contig, self.n_reads, read_names=self.read_names, unknown=self.unknown, evmu=pin(self.evmu),
                  model_n_bits=pin(self.model_n_bits), idx_rel_bits=pin(self.idx_rel_bits))
        t._owner = keep
        return t

    def view(self):
        v = TableView()
        v.n_rows = self.n_rows
        if self.pos is not None:                       # (a device-parsed table has its columns in a table slot only)
            v.pos, v.event_model_e4 = _ptr(self.pos), _ptr(self.evmu)
            v.event_idx = _ptr(self.event_idx)
        v.flags = _ptr(self.flags)
        if self.pos is not None:
            self._nbits_viewed = self.model_n_bits     # (kept: the view points into it)
            v.model_n_bits = _ptr(self._nbits_viewed)
            self._xrel_viewed = self.idx_rel_bits      # (likewise)
            v.idx_rel_bits = _ptr(self._xrel_viewed)
        v.n_seg = self.n_seg
        v.seg_row_begin, v.seg_read, v.seg_contig = _ptr(self.seg_row_begin), _ptr(self.seg_read), _ptr(self.seg_contig)
        v.n_reads = self.n_reads
        return v

    def slice_segments(self, s0, s1):
        """Sub-table of segments [s0, s1) (a shard); row indices restart at 0, read ids are kept."""
        r0, r1 = int(self.seg_row_begin[s0]), int(self.seg_row_begin[s1])
        # (the maker's bit column: whole bytes carry over when the cut falls on one, the bits of the rows behind the slice
        # cleared; otherwise the slice's flags are packed again when the column is asked for)
        bits = None
        if self._model_n_bits is not None and r0 % 8 == 0:
            bits = self._model_n_bits[r0 // 8:(r1 + 7) // 8]
            if r1 % 8 and r1 < self.n_rows:
                bits = bits.copy()
                bits[-1] &= (1 << (r1 % 8)) - 1
        # (the maker's relation column likewise: whole words on a cut at a multiple of eight rows, the slice's first row with no
        # row before it any more, the bits of the rows behind the slice cleared)
        rel = None
        if self._idx_rel_bits is not None and r0 % 8 == 0 and r1 > r0:
            rel = self._idx_rel_bits[r0 // 8:(r1 + 7) // 8].copy()
            rel[0] &= 0xFEFE
            if r1 % 8 and r1 < self.n_rows:
                rel[-1] &= ((1 << (r1 % 8)) - 1) * 0x0101
        return Table(self.pos[r0:r1], None, None, self.event_idx[r0:r1],
                     self.flags[r0:r1], self.seg_row_begin[s0:s1 + 1] - r0, self.seg_read[s0:s1],
                     self.seg_contig[s0:s1], self.n_reads, read_names=self.read_names, owner=self._owner,
                     evmu=self.evmu[r0:r1],
                     model_n_bits=bits, idx_rel_bits=rel)


class TextBlock(object):
    """A byte range of a file where the DMA engines can read it (what the device parser is given): mapped from the page cache
    and registered (mc_map_file_range: no copy by the CPU; MCALLER_READER=mmap), or -- the default, and where the mapping cannot
    be registered -- read into a block of the pinned host pool."""

    def __init__(self, path, lo, hi, n_threads=0):
        self.n_bytes = int(hi - lo)
        self._map = None
        self._mem = None
        if self.n_bytes and os.environ.get('MCALLER_READER', 'pread').startswith('mmap'):
            handle, ptr = C.c_void_p(), C.c_void_p()
            if lib().mc_map_file_range(path.encode('utf-8'), int(lo), int(hi), C.byref(handle), C.byref(ptr)) == 0:
                self._map = handle
                self.ptr = ptr.value
                self.array = np.frombuffer((C.c_char * self.n_bytes).from_address(self.ptr), dtype=np.uint8)
                return
        self._mem = PinnedArray((max(self.n_bytes, 1),), np.uint8)
        self.array = self._mem.array
        self.ptr = self._mem.ptr
        if self.n_bytes:
            check(lib().mc_read_file_range(path.encode('utf-8'), int(lo), int(hi), self.ptr, int(n_threads)))

    @property
    def mapped(self):
        return self._map is not None

    def token(self, off, n):
        return bytes(self.array[off:off + n]).decode('utf-8', 'surrogateescape')

    def __del__(self):
        try:
            if self._map is not None:
                self.array = None
                if os.environ.get('MCALLER_READER') != 'mmap_keep':      # (experiment: the mappings stay until the process ends)
                    lib().mc_unmap_file_range(self._map)
                self._map = None
        except Exception:       # noqa (interpreter shutdown)
            pass


def device_table(res, text):
    """Table whose columns the device parser has put into a table slot (mc_ctx_parse_end's result `res`, a DevParseResult;
    `text`: the TextBlock it was made from): the host side holds the segments, the flag column and the names only."""
    n, ns = int(res.n_rows), int(res.n_seg)
    t = Table.__new__(Table)
    t.pos = t.evmu = t.event_idx = None                # (on the device only)
    t.flags = _from_ptr(res.flags, n, np.uint8).copy()
    t._model_n_bits = None                             # (on the device only: kp_place wrote it with the flag column)
    t._idx_rel_bits = None                             # (likewise, with the index column)
    rows = _from_ptr(res.seg_row_begin, ns, np.int64)
    t.seg_row_begin = np.concatenate([rows, np.array([n], dtype=np.int64)])
    t.seg_contig = _from_ptr(res.seg_contig, ns, np.int32).copy()
    off, ln = _from_ptr(res.seg_name_off, ns, np.int64), _from_ptr(res.seg_name_len, ns, np.int32)
    ids, names, seg_read = {}, [], np.empty(ns, dtype=np.int32)
    for i in range(ns):                                # read ids in the order the names first appear, like the host parser
        name = text.token(int(off[i]), int(ln[i]))
        rid = ids.get(name)
        if rid is None:
            rid = ids[name] = len(names)
            names.append(name)
        seg_read[i] = rid
    t.seg_read = seg_read
    t.seg_name_start = _from_ptr(res.seg_name_start, ns, np.uint8).copy()
    t.n_reads, t.read_names = len(names), names
    uo, ul = _from_ptr(res.unknown_off, int(res.n_unknown), np.int64), _from_ptr(res.unknown_len, int(res.n_unknown), np.int32)
    t.unknown = [text.token(int(uo[i]), int(ul[i])) for i in range(int(res.n_unknown))]
    t._owner = None
    t.n_rows, t.n_seg = n, ns
    t.n_pieces = 0
    t.device_slot = None                               # set by Device.parse_end
    return t


def fastq_read_quality(path, n_threads=0):
    """Native FASTQ reader -> (keys: list of str, means: float64 array), one entry per record in file order."""
    L = lib()
    handle = C.c_void_p()
    if L.mc_fastq_read_quality(path.encode('utf-8'), int(n_threads), C.byref(handle)) != 0:
        raise ValueError(last_error())
    try:
        pool, off, mean = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = L.mc_fastq_view(handle, C.byref(pool), C.byref(off), C.byref(mean))
        return fastq_unpack(pool, off, mean, n)
    finally:
        L.mc_fastq_free(handle)


def fastq_unpack(pool, off, mean, n):
    """The layout of mc_fastq_view (and of mc_fastq_quality_view): a pool of keys with a newline behind each, n + 1 offsets, n means
    -> (keys: list of str, means: float64 array), copies."""
    if n <= 0:
        return [], np.zeros(0, dtype=np.float64)
    offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_int64)), shape=(n + 1,))
    text = C.string_at(pool, int(offs[n])).decode('utf-8')
    means = np.ctypeslib.as_array(C.cast(mean, C.POINTER(C.c_double)), shape=(n,)).copy()
    return text.split('\n')[:n], means


def fastq_records_host(text):
    """The record rules of csrc/mc_fastqrec.h run on the CPU over `text` (bytes), no GPU (mc_fastq_records_host): what the device
    reader is held against.  -> (keys, means, None), or (None, None, dict(reason=MC_FASTQ_DECLINE_*, line=0-based, text=str)) where
    the rules decline."""
    L = lib()
    text = bytes(text)
    handle, status = C.c_void_p(), C.c_int32()
    check(L.mc_fastq_records_host(text, len(text), C.byref(handle), C.byref(status)))
    if status.value != 0:
        reason, line = C.c_int32(), C.c_int64()
        L.mc_fastq_records_host_decline(C.byref(reason), C.byref(line))
        return None, None, dict(reason=reason.value, line=line.value, text=last_error())
    try:
        pool, off, mean = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = L.mc_fastq_view(handle, C.byref(pool), C.byref(off), C.byref(mean))
        return fastq_unpack(pool, off, mean, n) + (None,)
    finally:
        L.mc_fastq_free(handle)


def eventalign_read_cuts(path, n_parts, lo=None, hi=None):
    """Byte offsets (n_parts + 1) cutting an eventalign file (or its byte range [lo, hi)) at the first lines of reads,
    pieces of similar size."""
    cuts = np.zeros(n_parts + 1, dtype=np.int64)
    if lo is None and hi is None:
        check(lib().mc_eventalign_read_cuts(path.encode('utf-8'), int(n_parts), _ptr(cuts)))
    else:
        check(lib().mc_eventalign_read_cuts_range(path.encode('utf-8'), int(lo or 0), int((1 << 62) if hi is None else hi),
                                                  int(n_parts), _ptr(cuts)))
    return [int(c) for c in cuts]


def eventalign_read_cuts_at(path, want, lo, hi):
    """Byte offsets cutting [lo, hi) at the first lines of the reads at or behind the offsets `want` (ascending): [lo, ..., end]."""
    want = np.ascontiguousarray(want, dtype=np.int64)
    cuts = np.zeros(len(want) + 2, dtype=np.int64)
    check(lib().mc_eventalign_read_cuts_at(path.encode('utf-8'), int(lo), int(hi), _ptr(want), len(want), _ptr(cuts)))
    return [int(c) for c in cuts]


def eventalign_consumed_range(path, startline, endline):
    """[lo, hi): the bytes the reference's batch loop reads for (startline, endline) (extract_contexts.py:141-148)."""
    lo, hi = C.c_int64(0), C.c_int64(0)
    check(lib().mc_eventalign_consumed_range(path.encode('utf-8'), int(startline), int(endline), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def parse_eventalign(path, startline, endline, contig_names, n_threads=0, exact_range=False):
    """Native parser -> Table over the library's buffers (no copy; freed with the Table)."""
    L = lib()
    arr = (C.c_char_p * max(1, len(contig_names)))()
    for i, n in enumerate(contig_names):
        arr[i] = n.encode('utf-8')
    handle = C.c_void_p()
    fn = L.mc_parse_eventalign_range if exact_range else L.mc_parse_eventalign
    check(fn(path.encode('utf-8'), int(startline), int(endline), arr, len(contig_names), int(n_threads), C.byref(handle)))
    owner = _Parsed(handle)          # the columns stay in the library's buffers (no copy); freed with the Table
    v = TableView()
    check(L.mc_parsed_view(handle, C.byref(v)))
    n, ns = v.n_rows, v.n_seg
    names = [L.mc_parsed_read_name(handle, i).decode('utf-8', 'surrogateescape') for i in range(v.n_reads)]
    unknown = [L.mc_parsed_unknown_name(handle, i).decode('utf-8', 'surrogateescape')
               for i in range(L.mc_parsed_n_unknown(handle))]
    t = Table(_from_ptr(v.pos, n, np.int32), None, None,
              _from_ptr(v.event_idx, n, np.int32), _from_ptr(v.flags, n, np.uint8),
              _from_ptr(v.seg_row_begin, ns + 1, np.int64), _from_ptr(v.seg_read, ns, np.int32),
              _from_ptr(v.seg_contig, ns, np.int32), v.n_reads, read_names=names, unknown=unknown, owner=owner,
              evmu=_from_ptr(v.event_model_e4, 2 * n, np.int32).reshape(-1, 2),
              model_n_bits=_from_ptr(v.model_n_bits, (n + 7) // 8, np.uint8),
              idx_rel_bits=_from_ptr(v.idx_rel_bits, (n + 7) // 8, np.uint16))
    t.n_pieces = int(L.mc_parsed_n_pieces(handle))
    return t


class _Parsed(object):
    """Owns a mc_parsed handle: the Table built over it keeps it alive."""

    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle:
                lib().mc_parsed_free(self.handle)
                self.handle = None
        except Exception:
            pass


def make_ref_view(arrays):
    """arrays: dict from MarkedReference.device_arrays() -> (RefView, keepalive)."""
    v = RefView()
    v.n_contigs = len(arrays['contig_len'])
    v.contig_len, v.seq_off, v.seq = _ptr(arrays['contig_len']), _ptr(arrays['seq_off']), _ptr(arrays['seq'])
    v.word_off, v.mbits_fwd, v.mbits_rev = _ptr(arrays['word_off']), _ptr(arrays['mbits_fwd']), _ptr(arrays['mbits_rev'])
    v.n_seq_bytes = len(arrays['seq'])
    v.n_words = len(arrays['mbits_fwd'])
    return v


def _cstr_array(strings):
    arr = (C.c_char_p * max(1, len(strings)))()
    for i, s in enumerate(strings):
        arr[i] = s if isinstance(s, bytes) else str(s).encode('utf-8', 'surrogateescape')
    return arr


class DiffsFormatter(object):
    """mc_format_diffs over one (records, table, reference): rows of records [first, stop) as bytes."""

    def __init__(self, rec, table, ref_arrays, contig_names, read_qual_txt, k, label_meth, label_unmeth,
                 submodel_of_char, tail_chrom=None):
        self._keep = (rec, table, ref_arrays)
        self._rv, self._tv, self._fv = rec.view(), table.view(), make_ref_view(ref_arrays)
        self._rv.capacity = rec.n
        self._contigs, self._reads = _cstr_array(contig_names), _cstr_array(table.read_names)
        self._quals = _cstr_array(read_qual_txt)
        self._soc = np.ascontiguousarray(submodel_of_char, dtype=np.uint8)
        self._tail = tail_chrom.encode('utf-8', 'surrogateescape') if tail_chrom is not None else None
        self._labels = label_meth.encode(), label_unmeth.encode()
        a = FormatArgs()                 # (its pointer fields are plain addresses: everything they point at is kept in self)
        a.rec, a.n_records, a.k = C.addressof(self._rv), rec.n, k
        a.table, a.ref = C.addressof(self._tv), C.addressof(self._fv)
        a.contig_names, a.read_names, a.read_qual_txt = (C.addressof(s) for s in (self._contigs, self._reads, self._quals))
        a.tail_chrom, a.label_meth, a.label_unmeth = (C.cast(s, C.c_void_p) for s in (self._tail,) + self._labels)
        a.submodel_of_char = _ptr(self._soc)
        self._args = a

    def rows(self, first, n_threads=0):
        """-> (rows as a bytes-like object, number of rows, stop): stop < n means record `stop` needs the host's own handling.
        The rows stay in the buffer the library made (a one-base motif writes a gigabyte of them per 10^8 events: no copy into a
        bytes object here, none when they are joined -- whoever writes them hands the buffer to write())."""
        text, nb, nr, stop = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().mc_format_diffs(C.byref(self._args), int(first), int(n_threads), C.byref(text), C.byref(nb),
                                    C.byref(nr), C.byref(stop)))
        return LibBuffer(text, nb.value), nr.value, stop.value


class LibBuffer(object):
    """Bytes the library allocated (mc_free releases them when this object goes): `view` is a memoryview over them."""

    def __init__(self, ptr, n):
        self._ptr, self.n = ptr, int(n)
        self.view = memoryview((C.c_char * self.n).from_address(ptr.value)).cast('B') if self.n else memoryview(b'')

    def __len__(self):
        return self.n

    def __bytes__(self):
        return self.view.tobytes()

    def __del__(self):
        try:
            if self._ptr is not None and self._ptr.value:
                self.view.release()
                lib().mc_free(self._ptr)
        except Exception:       # noqa (interpreter shutdown)
            pass
        self._ptr = None


class RowText(object):
    """The rows of a pass as the device wrote them (mc_last_row_text): `view` is a memoryview over the pinned block, `n_rows` the
    rows in it; release() (or the end of this object) gives the block back to the context -- the text must have been written by then."""

    def __init__(self, device, ptr, n_bytes, n_rows, block):
        self._dev, self._block = device, int(block)        # (the Device, not its context: a block outlives neither)
        self.n, self.n_rows = int(n_bytes), int(n_rows)
        self.view = memoryview((C.c_char * self.n).from_address(ptr)).cast('B') if self.n else memoryview(b'')

    def __len__(self):
        return self.n

    def __bytes__(self):
        return self.view.tobytes()

    def release(self):
        if self._block >= 0:
            block, self._block = self._block, -1
            self.view.release()
            self.view = memoryview(b'')
            self.n = 0
            self._dev._row_text_release(block)

    def __del__(self):
        try:
            self.release()
        except Exception:       # noqa (interpreter shutdown)
            pass


def repr_double(x):
    buf = C.create_string_buffer(40)
    lib().mc_repr_double(float(x), buf)
    return buf.value.decode()


def tstat(n, mean, var):
    """t and log10 p of a one-sample t-test from (rows, mean, sample variance) by mc_tstat.h's host build (mc_tstat).
    -> (status bits, t, log10 p); the bits: include/mcaller_hip.h."""
    t, l = C.c_double(), C.c_double()
    st = lib().mc_tstat(float(n), float(mean), float(var), C.byref(t), C.byref(l))
    return st, t.value, l.value


def gff_site_moments(p):
    """(status bits, np.mean(p), np.var(p, ddof=1), np.std(p, ddof=1) / np.sqrt(len(p))) by mc_npsum.h's host build: NumPy's own
    order of additions (mc_gff_site_moments)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.zeros(3)
    st = lib().mc_gff_site_moments(p.ctypes.data, len(p), out.ctypes.data)
    return st, out[0], out[1], out[2]


def gff_site_stats(p, frac):
    """(status bits, fracLow, fracUp, 100 * mean) of make_bed --gff --vo by mc_npsum.h's host build (mc_gff_site_stats)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.zeros(3)
    st = lib().mc_gff_site_stats(p.ctypes.data, len(p), float(frac), out.ctypes.data)
    return st, out[0], out[1], out[2]


def gff_site_text(p, frac):
    """';fracLow=..;fracUp=..;identificationQv=..' as the kernels print it (mc_gff_site_text), or None where the device declines."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    buf = C.create_string_buffer(160)
    n = lib().mc_gff_site_text(p.ctypes.data, len(p), float(frac), buf, 160)
    return buf.raw[:n].decode('ascii') if n >= 0 else None


def npsum_se(var, n):
    """sqrt(var) / sqrt(n) with mc_npsum.h's correctly rounded square root (host build)."""
    return lib().mc_npsum_se(float(var), float(n))


def tstat_round3(v):
    """np.round(v, 3) by mc_tstat.h's host build."""
    return lib().mc_tstat_round3(float(v))


def tstat_tie(v, err):
    """Can np.round(h, 3) differ from np.round(v, 3) for an h within err of v?  (mc_tstat.h's tie test, host build)"""
    return bool(lib().mc_tstat_tie(float(v), float(err)))


def tstat_site(rows):
    """The two values make_bed -p prints for an entry with the value rows `rows` ([n][values], the last value dropped), by the
    host build of what the kernels do (mc_tstat_site) -> (status bits, round3(max t), round3(sum -log10 p))."""
    X = np.ascontiguousarray(rows, dtype=np.float64)
    out = np.zeros(2, dtype=np.float64)
    st = lib().mc_tstat_site(X.ctypes.data, X.shape[0], X.shape[1], out.ctypes.data)
    return st, float(out[0]), float(out[1])


def hypergeom_tail(N, K, d, k):
    """P(X >= k) for X ~ Hypergeometric(N, K, d) and the derived bound on its error, by mc_hypergeom.h's host build.  Scalars
    -> (status, tail, err) (mc_hypergeom_tail); four arrays of one length -> (tail float64 [n], err float64 [n]), NaN where the
    arguments are out of range (mc_hypergeom_tail_many)."""
    if np.ndim(N) == 0:
        t, e = C.c_double(), C.c_double()
        st = lib().mc_hypergeom_tail(int(N), int(K), int(d), int(k), C.byref(t), C.byref(e))
        return st, t.value, e.value
    N, K, d, k = (np.ascontiguousarray(a, dtype=np.int64) for a in (N, K, d, k))
    if not (N.ndim == 1 and N.shape == K.shape == d.shape == k.shape):
        raise ValueError('hypergeom_tail: four arrays of one length')
    tail, err = np.zeros(len(N)), np.zeros(len(N))
    rc = lib().mc_hypergeom_tail_many(N.ctypes.data, K.ctypes.data, d.ctypes.data, k.ctypes.data, len(N), tail.ctypes.data, err.ctypes.data)
    if rc:
        raise ValueError('mc_hypergeom_tail_many: %d' % rc)
    return tail, err


def hypergeom_masses(N, K, d):
    """The bucket masses behind all 101 tails of X ~ Hypergeometric(N, K, d) and the derived bound on their summed error, by
    mc_hypergeom.h's host build: P(X >= k_min(d, j)) = mass[j + 1:].sum().  Scalars -> (status, mass float64 [102], err)
    (mc_hypergeom_masses); three arrays of one length -> (mass float64 [n, 102], err float64 [n]), NaN where the arguments are out
    of range (mc_hypergeom_masses_many)."""
    B = _K['MC_HYPERGEOM_BUCKETS']
    if np.ndim(N) == 0:
        mass, e = np.zeros(B), C.c_double()
        st = lib().mc_hypergeom_masses(int(N), int(K), int(d), mass.ctypes.data, C.byref(e))
        return st, mass, e.value
    N, K, d = (np.ascontiguousarray(a, dtype=np.int64) for a in (N, K, d))
    if not (N.ndim == 1 and N.shape == K.shape == d.shape):
        raise ValueError('hypergeom_masses: three arrays of one length')
    mass, err = np.zeros((len(N), B)), np.zeros(len(N))
    rc = lib().mc_hypergeom_masses_many(N.ctypes.data, K.ctypes.data, d.ctypes.data, len(N), mass.ctypes.data, err.ctypes.data)
    if rc:
        raise ValueError('mc_hypergeom_masses_many: %d' % rc)
    return mass, err


def fisher_exact(K1, n1, K2, n2):
    """log10 of the two-sided p of Fisher's exact test on K1 of n1 against K2 of n2, its derived bound and the status bits
    (MC_FISHER_*), by mc_fisher.h's host build.  Scalars -> (status, log10_p, bound) (mc_fisher_exact); four arrays of one
    length -> (log10_p float64 [n], bound float64 [n], status int32 [n]) (mc_fisher_exact_many)."""
    if np.ndim(K1) == 0:
        l, b, st = C.c_double(), C.c_double(), C.c_int32()
        rc = lib().mc_fisher_exact(int(K1), int(n1), int(K2), int(n2), C.byref(l), C.byref(b), C.byref(st))
        if rc != 0:
            raise ValueError('mc_fisher_exact: %d' % rc)
        return int(st.value), l.value, b.value
    K1, n1, K2, n2 = (np.ascontiguousarray(a, dtype=np.int64) for a in (K1, n1, K2, n2))
    if not (K1.ndim == 1 and K1.shape == n1.shape == K2.shape == n2.shape):
        raise ValueError('fisher_exact: four arrays of one length')
    l, b, st = np.zeros(len(K1)), np.zeros(len(K1)), np.zeros(len(K1), dtype=np.int32)
    rc = lib().mc_fisher_exact_many(K1.ctypes.data, n1.ctypes.data, K2.ctypes.data, n2.ctypes.data, len(K1), l.ctypes.data, b.ctypes.data,
                                    st.ctypes.data)
    if rc != 0:
        raise ValueError('mc_fisher_exact_many: %d' % rc)
    return l, b, st


def fisher_select(w, w_obs, steps):
    """mc_fisher.h's selection predicate on a weight beside the observed one, both at most `steps` steps from the mode
    -> (selected, within its error of the factor 1 + 10^-7)."""
    r = lib().mc_fisher_select(float(w), float(w_obs), float(steps))
    return bool(r & 1), bool(r & 2)


def bh_adjust(L, bound):
    """The Benjamini-Hochberg adjustment of one column of log10 p (NaN: an untested row) by mc_bh.h's host build
    -> (Q float64 [n]: log10 q, rounded float64 [n]: np.round(0.0 - Q, 3), status: MC_BH_* bits)."""
    L, bound = np.ascontiguousarray(L, dtype=np.float64), np.ascontiguousarray(bound, dtype=np.float64)
    if not (L.ndim == 1 and L.shape == bound.shape):
        raise ValueError('bh_adjust: two arrays of one length')
    Q, rounded, st = np.zeros(len(L)), np.zeros(len(L)), C.c_int32()
    rc = lib().mc_bh_adjust(L.ctypes.data, bound.ctypes.data, len(L), Q.ctypes.data, rounded.ctypes.data, C.byref(st))
    if rc != 0:
        raise ValueError('mc_bh_adjust: %d' % rc)
    return Q, rounded, int(st.value)


def curcombine(L, bound, log10c):
    """compare_currents' Bonferroni combination of one test's columns (L: their unrounded log10 p, bound: the bounds on them) by
    mc_curcombine.h's host build -> (combined log10 p, np.round(0.0 - L, 3), the bound on L, status: CC_* bits)."""
    L, bound = np.ascontiguousarray(L, dtype=np.float64), np.ascontiguousarray(bound, dtype=np.float64)
    if not (L.ndim == 1 and L.shape == bound.shape and len(L) >= 1):
        raise ValueError('curcombine: two arrays of one length, at least 1')
    out, b, st = np.zeros(2), C.c_double(), C.c_int32()
    rc = lib().mc_curcombine(L.ctypes.data, bound.ctypes.data, len(L), float(log10c), out.ctypes.data, C.byref(b), C.byref(st))
    if rc != 0:
        raise ValueError('mc_curcombine: %d' % rc)
    return float(out[0]), float(out[1]), float(b.value), int(st.value)


def site_cluster(values, metric='correlation'):
    """cluster_sites' split of one site (values [n, c], n <= 1024) by mc_linkage.h's host build -> None when fewer than 2 rows are
    usable, else (labels: int32 [n], 0 a flat row, 1 or 2; h_top; h_sub)."""
    X = np.ascontiguousarray(values, dtype=np.float64)
    if X.ndim != 2 or metric not in CLU_METRIC:
        raise ValueError('site_cluster: values [n, c] and a metric of correlation or euclidean')
    labels, out = np.zeros(X.shape[0], dtype=np.int32), np.zeros(3)
    rc = lib().mc_site_cluster_host(X.ctypes.data, X.shape[0], X.shape[1], CLU_METRIC[metric], labels.ctypes.data, out.ctypes.data)
    if rc == 1:
        return None
    if rc != 0:
        raise ValueError('mc_site_cluster_host: %d' % rc)
    return labels, float(out[0]), float(out[1])


def pair_phi(n11, n10, n01, n00):
    """phase_reads' phi of one 2 x 2 table by mc_pairphase.h's host build -> None when a margin is zero, else (phi, np.round(phi, 3))."""
    phi, rounded = C.c_double(), C.c_double()
    rc = lib().mc_pair_phi(int(n11), int(n10), int(n01), int(n00), C.byref(phi), C.byref(rounded))
    if rc == 1:
        return None
    if rc != 0:
        raise ValueError('mc_pair_phi: %d' % rc)
    return phi.value, rounded.value


def site_ari(n1, n2, m1, m2):
    """The adjusted Rand index of (cluster, methylated) by mc_linkage.h's host build (nan: counts that are none)."""
    return lib().mc_site_ari_host(int(n1), int(n2), int(m1), int(m2))


def hypergeom_round4(v):
    """np.round(v, 4) by mc_hypergeom.h's host build."""
    return lib().mc_hypergeom_round4(float(v))


def hypergeom_tie4(v, err):
    """Can np.round(h, 4) differ from np.round(v, 4) for an h within err of v?  (mc_hypergeom.h's tie test, host build)"""
    return bool(lib().mc_hypergeom_tie4(float(v), float(err)))


def parse_double(token):
    """float(token) by mc_decimal.h's host build (mc_parse_double): the double, or None for a form that header declines.
    `token`: bytes (a str is encoded as latin-1, so that every character is one byte)."""
    if isinstance(token, str):
        token = token.encode('latin-1', 'replace')
    out = C.c_double()
    return out.value if lib().mc_parse_double(token, len(token), C.byref(out)) else None


def repr_double_rowtext(x):
    """repr(x) by the device row writer's digit generation, built for the host (None: a double it does not print)."""
    buf = C.create_string_buffer(40)
    n = lib().mc_repr_double_rowtext(float(x), buf)
    return buf.value.decode() if n >= 0 else None


def repr_fixed4(d):
    buf = C.create_string_buffer(40)
    lib().mc_repr_fixed4(int(d), buf)
    return buf.value.decode()


class Records(object):
    """Host buffers for flush records (mc_calls_view)."""

    def __init__(self, capacity, k):
        self.k = k
        self.capacity = int(capacity)
        c = max(1, self.capacity)
        self.feats = np.zeros(c * k, dtype=np.float64)
        self.site_pos = np.zeros(c, dtype=np.int32)
        self.site_seg = np.zeros(c, dtype=np.int32)
        self.close_row = np.zeros(c, dtype=np.int64)
        self.info = np.zeros(c, dtype=np.uint32)
        self.prob = np.full(c, np.nan, dtype=np.float64)
        self.n = 0

    def view(self):
        v = CallsView()
        v.capacity = self.capacity
        v.prob = _ptr(self.prob)
        v.copy_out_bytes = int(self.copy_out_bytes)
        narrow = self._narrow is not None and self._site_pos is None       # narrow records as mc_wait_records sent them
        if narrow:
            close_lo, pos_lo, info_lo, info_next, runs = self._narrow
            v.close_lo16, v.pos_lo16, v.info_lo16, v.info_next = _ptr(close_lo), _ptr(pos_lo), _ptr(info_lo), _ptr(info_next)
            v.runs, v.n_runs = _ptr(runs), len(runs) // 4
        else:
            v.site_pos, v.site_seg, v.info = _ptr(self.site_pos), _ptr(self.site_seg), _ptr(self.info)
        if self._feats is None and self._packed is not None:           # slot means as mc_wait_records sent them
            lo, hi, wide = self._packed
            v.feats_lo32, v.feats_hi32, v.feats_wide, v.n_wide = _ptr(lo), _ptr(hi), _ptr(wide), len(hi)
        else:
            v.feats = _ptr(self.feats)
        if narrow:
            pass
        elif self._close_row is not None or self._close_row32 is None:
            v.close_row = _ptr(self.close_row)
        else:
            v.close_row32 = _ptr(self._close_row32)
        if self._compacted:
            v.compacted, v.n_call_rows = 1, int(self._n_calls)
            if self._call_row is not None:
                v.call_row = _ptr(self._call_row)
        return v

    @classmethod
    def from_view(cls, v, n, k, owner):
        """Zero-copy wrap of library-owned buffers (valid until the next call on the owning context)."""
        r = cls.__new__(cls)
        r.k, r.capacity, r.n, r._owner = k, n, n, owner
        if v.feats:
            r.feats = _from_ptr(v.feats, n * k, np.float64)
        r.copy_out_bytes = int(v.copy_out_bytes)
        if v.close_lo16:                     # narrow records (mc_calls_view.close_lo16): the four columns are rebuilt on first use
            r._narrow = (_from_ptr(v.close_lo16, n, np.uint16), _from_ptr(v.pos_lo16, n, np.uint16), _from_ptr(v.info_lo16, n, np.uint16),
                         _from_ptr(v.info_next, n, np.uint8), _from_ptr(v.runs, 4 * int(v.n_runs), np.int32))
        else:
            r.site_pos = _from_ptr(v.site_pos, n, np.int32)
            r.site_seg = _from_ptr(v.site_seg, n, np.int32)
            if v.close_row:
                r._close_row = _from_ptr(v.close_row, n, np.int64)
            else:                            # mc_wait_records on tables below 2^31 - 1 rows: 32-bit closing rows
                r._close_row32 = _from_ptr(v.close_row32, n, np.int32)
            r.info = _from_ptr(v.info, n, np.uint32)
        if v.compacted:                      # mc_wait_records: means / probabilities of the calls only, compacted
            m = int(v.n_call_rows)
            r._compacted = True
            if v.call_row:
                r._call_row = _from_ptr(v.call_row, n, np.int32)
            r._n_calls = m
            if v.feats:
                r.feats = _from_ptr(v.feats, m * k, np.float64)
            else:                            # packed slot means (mc_calls_view.feats_lo32): unpacked on first use
                r._packed = (_from_ptr(v.feats_lo32, m * k, np.int32), _from_ptr(v.feats_hi32, int(v.n_wide), np.uint32),
                             _from_ptr(v.feats_wide, m, np.uint8))
            r.prob = _from_ptr(v.prob, m, np.float64)
        else:
            r.prob = _from_ptr(v.prob, n, np.float64)
        return r

    # closing rows, call rows, slot means: columns mc_wait_records does not send in full (mc_calls_view) are rebuilt on first use
    _close_row = _close_row32 = _call_row = _feats = _packed = None
    _site_pos = _site_seg = _info = _narrow = None
    _compacted = False
    copy_out_bytes = 0          # bytes the pass's records took on their way to the host (mc_wait_records), whichever layout

    @property
    def n_runs(self):
        """Entries of the run list of narrow records as they arrived; 0: the columns travelled in full."""
        return len(self._narrow[4]) // 4 if self._narrow is not None else 0

    def _widen(self):
        """Narrow records: site_pos, site_seg, info and close_row in full (mc_records_expand), once."""
        if self._narrow is not None and self._site_pos is None:
            n = max(1, int(self.n))
            pos, seg, info, close = (np.empty(n, dtype=t) for t in (np.int32, np.int32, np.uint32, np.int64))
            v = self.view()
            check(lib().mc_records_expand(C.byref(v), int(self.n), _ptr(pos), _ptr(seg), _ptr(info), _ptr(close)))
            self._site_seg, self._info, self._close_row, self._site_pos = seg, info, close, pos

    def end_segments(self):
        """(segment of the first record, of the last): narrow records say so in their run list's first and last entries."""
        if self._narrow is not None and self._site_pos is None:
            runs = self._narrow[4]
            return int(runs[1]), int(runs[-3])
        return int(self.site_seg[0]), int(self.site_seg[self.n - 1])

    @property
    def site_pos(self):
        self._widen()
        return self._site_pos

    @site_pos.setter
    def site_pos(self, a):
        self._site_pos = a

    @property
    def site_seg(self):
        self._widen()
        return self._site_seg

    @site_seg.setter
    def site_seg(self, a):
        self._site_seg = a

    @property
    def info(self):
        self._widen()
        return self._info

    @info.setter
    def info(self, a):
        self._info = a

    @property
    def feats(self):
        """Slot means, k per row of feats / prob (row-major, flat)."""
        if self._feats is None and self._packed is not None:
            out = np.empty(max(1, self._n_calls * self.k), dtype=np.float64)
            v = self.view()
            check(lib().mc_calls_expand(C.byref(v), int(self.n), int(self.k), None, None, _ptr(out)))
            self._feats = out[:self._n_calls * self.k]
        return self._feats

    @feats.setter
    def feats(self, a):
        self._feats = a

    @property
    def close_row(self):
        self._widen()
        if self._close_row is None and self._close_row32 is not None:
            self._close_row = self._close_row32.astype(np.int64)
        return self._close_row

    @close_row.setter
    def close_row(self, a):
        self._close_row = a

    @property
    def call_row(self):
        """None: feats / prob have one row per record.  Else the row of every record in feats / prob (-1: MC_I_TOO_MANY)."""
        if self._call_row is None and self._compacted:
            keep = (self.info[:self.n] & I_TOO_MANY) == 0
            rows = np.cumsum(keep, dtype=np.int64) - 1
            rows[~keep] = -1
            self._call_row = rows.astype(np.int32)
        return self._call_row

    @call_row.setter
    def call_row(self, a):
        self._call_row = a
        self._compacted = a is not None

    def count(self, n, seg_read=None, pos_marks=None):
        """mc_count_records over records [0, n): -> ((too many skips, skips included, multiple M) or None, ascending, smallest site
        position of a call, largest + 1); pos_marks: uint8 array, the calls' positions below its length are marked."""
        v = self.view()
        counts = np.zeros(3, dtype=np.int64)
        asc, lo, top = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        if seg_read is not None:
            seg_read = np.ascontiguousarray(seg_read, dtype=np.int32)
        check(lib().mc_count_records(C.byref(v), int(n), _ptr(seg_read) if seg_read is not None else None,
                                     len(seg_read) if seg_read is not None else 0, _ptr(counts) if seg_read is not None else None,
                                     C.byref(asc), _ptr(pos_marks) if pos_marks is not None else None,
                                     len(pos_marks) if pos_marks is not None else 0, C.byref(lo), C.byref(top)))
        return (tuple(int(c) for c in counts) if seg_read is not None else None), bool(asc.value), int(lo.value), int(top.value)

    @property
    def n_calls(self):
        """Rows of feats / prob."""
        return self._n_calls if self._compacted else self.n

    def by_record(self):
        """A copy with one feats / prob row per record (zeros / NaN for the MC_I_TOO_MANY records of a compacted view)."""
        if self.call_row is None:
            return self
        n, k = self.n, self.k
        r = Records(n, k)
        r.n = n
        for name in ('site_pos', 'site_seg', 'close_row', 'info'):
            getattr(r, name)[:n] = getattr(self, name)[:n]
        kept = self.call_row[:n] >= 0
        rows = self.call_row[:n][kept]
        r.feats.reshape(-1, k)[:n][kept] = self.feats.reshape(-1, k)[rows]
        r.prob[:n][kept] = self.prob[rows]
        return r


def twosample(x, y):
    """The nine values of a compare_genomes row for the samples x and y by mc_twosample.h's host build (mc_twosample)
    -> (status bits, float64 [9] in TW_NAMES' order, float64 [9]: the bound on |device - host| of each before rounding)."""
    import numpy as np
    x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y))
    out, bound, st = np.zeros(9), np.zeros(9), C.c_int32()
    rc = lib().mc_twosample(x.ctypes.data, len(x), y.ctypes.data, len(y), out.ctypes.data, bound.ctypes.data, C.byref(st))
    if rc != 0:
        raise ValueError('mc_twosample: bad arguments')
    return st.value, out, bound


def twosample_log10_2sf(z):
    """log10(2 * norm.sf(z)), z >= 0, by mc_twosample.h's host build."""
    return lib().mc_twosample_log10_2sf(float(z))


def twosample_log10_kolmogorov(lam):
    """log10(scipy.special.kolmogorov(lam)) by mc_twosample.h's host build."""
    return lib().mc_twosample_log10_kolmogorov(float(lam))
