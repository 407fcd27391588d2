"""One table to rows: what stands between a parsed eventalign table and the reference's output (extract_contexts.py:110-303).

`prepare` / `prepare_table` mark the contigs and look up the read qualities, `compute` uploads and runs the HIP path,
`Finisher` turns the flush records into rows, counters and train dicts; the names at a cut of the file (`cut_names`,
`head_contig`) and the writers are here too.  Nothing here knows about shards (stream.py) or the drop-in (extract_contexts.py).
"""
import numpy as np

from . import _lib
from .device import get_device
from .refmark import MarkedReference, revcomp, strand

_I = _lib


def base_models(base, twobase=False):
    """Sub-model key for a context's two centre characters (extract_contexts.py:99-106)."""
    if base == 'A' and twobase:
        return {'MG': 'MG', 'MC': 'MH', 'MA': 'MH', 'MT': 'MH', 'MM': 'MH', 'MH': 'MH', 'AT': 'MH', 'AC': 'MH',
                'AG': 'MG', 'AA': 'MH', 'AM': 'MH'}
    base_model = {'M' + nextb: 'general' for nextb in ['A', 'C', 'G', 'T', 'M']}
    base_model.update({'A' + nextb: 'general' for nextb in ['A', 'C', 'G', 'T', 'M']})
    base_model.update({'T' + nextb: 'general' for nextb in ['A', 'C', 'G', 'T', 'M']})
    return base_model


def writefi(data, fi):
    """Append rows to the tmp file (extract_contexts.py:83-86)."""
    with open(fi, 'a') as outfi:
        for entry in data:
            outfi.write('\t'.join(entry) + '\n')


def write_text(blob, fi):
    """writefi for rows that are already text."""
    with open(fi, 'ab') as outfi:
        outfi.write(blob)


def fmt_float(x):
    """str(np.float64): shortest round-trip repr (what the reference's str(diff) prints)."""
    return repr(float(x))


def round2(p):
    """np.round(p, 2) (extract_contexts.py:207)."""
    return float(np.round(np.float64(p), 2))


class Prepared(object):
    """Everything the kernels and the formatter need for one (tsv byte range, reference, marking)."""
    pass


def _lookup_quality(read2qual, name):
    try:
        return read2qual[name]                                     # extract_contexts.py:163-166
    except KeyError:
        return read2qual[name.split(':')[0].split('_')[0]]


def prepare(tsv_input, fasta_input, read2qual, startline, endline, base, motif, positions_list, n_threads=0,
            exact_range=False, ref=None, quiet=False):
    """Parse + mark: the host-side pre-pass.  Returns a Prepared; `fatal` holds the exception the
    reference would hit at table row `len(table)` (the table is cut there).  `ref`: a MarkedReference to go on
    with (the shards of one file share it); quiet: the "could not find sequence" lines are kept in P.messages
    instead of being printed."""
    P = Prepared()
    if ref is None:
        ref = MarkedReference(fasta_input, base, motif, positions_list)
    table = _lib.parse_eventalign(tsv_input, startline, endline, ref.names, n_threads, exact_range=exact_range)
    return prepare_table(P, table, ref, read2qual, quiet)


def prepare_table(P, table, ref, read2qual, quiet=False):
    """The part of `prepare` behind the parser: contigs marked as they first appear, read qualities looked up.  `table`: from
    the host parser, or made on the device (Device.parse_end)."""
    P.messages = ['Error: could not find sequence for reference contig ' + name for name in table.unknown]   # :159
    if not quiet:
        for line in P.messages:
            print(line)
    P.fatal = None
    qual_obj = [None] * table.n_reads
    cut_seg = None
    for seg in range(table.n_seg):
        cid, rid = int(table.seg_contig[seg]), int(table.seg_read[seg])
        try:
            if cid not in ref.meth:
                ref.mark(cid)                                                    # :154-157 (may print + exit)
            if qual_obj[rid] is None:
                qual_obj[rid] = _lookup_quality(read2qual, table.read_names[rid])
        except (SystemExit, Exception) as e:                                     # noqa
            P.fatal = e
            cut_seg = seg
            break
    if cut_seg is not None and table.pos is not None:      # (a device-parsed table is only ever streamed: fatal sends the file to the one-table path)
        table = table.slice_segments(0, cut_seg)
    P.ref, P.table, P.qual_obj = ref, table, qual_obj
    P.qual = np.array([float(q) if q is not None else np.nan for q in qual_obj], dtype=np.float64)
    return P


def submodel_setup(modelset, base):
    """-> (base_model table, [weights...], key -> index, uint8[256] context[k] char -> index or 255)."""
    table = base_models(base, modelset.twobase)
    keys = modelset.keys()
    index = {key: i for i, key in enumerate(keys)}
    soc = np.full(256, 255, dtype=np.uint8)
    for c in range(256):
        two = 'M' + chr(c)
        if two in table and table[two] in index:
            soc[c] = index[table[two]]
    return table, [modelset.models[key] for key in keys], index, soc


def compute(P, k, skip_thresh, qual_thresh, modelset, base, train, device=None, tail_contig=-1):
    """Upload + run the HIP path.  Returns (records, info dict)."""
    dev = device if device is not None else get_device()
    dev.set_reference(P.ref.device_arrays())
    dev.upload_table(P.table)
    dev.set_read_quality(P.qual)
    if not train:
        _, weights, _, soc = submodel_setup(modelset, base)
        dev.set_classifier(weights, soc)
    rec = dev.extract(k, skip_thresh, qual_thresh, tail_contig=tail_contig, score=not train)
    return rec


class Finisher(object):
    """Flush records -> the reference's rows, counters and train dicts, in record (= file) order.

    Predict mode: the rows come with the records when the device wrote them (streamed shards: mc_rowtext.hip), else they are
    written by the native formatter (mc_format_diffs, all host cores); a record it hands
    back (context leaving the contig, unscored, unknown sub-model key: the reference's exit/crash paths) goes through
    `_one`, the literal per-record transcription of extract_contexts.py:179-239, which train mode uses throughout
    (it has to build the Python lists the caller trains on)."""

    def __init__(self, P, k, base, train, modelset=None, pos_label=None, device=None, tail_chrom=None):
        self.P, self.k, self.base, self.train = P, k, base, train
        self.pos_label = pos_label
        self.device = device
        self.tail_chrom = tail_chrom
        if not train:
            self.table, _, self.model_index, self.soc = submodel_setup(modelset, base)
            self.model_keys = modelset.keys()
        else:
            self.table = base_models(base, False)                                 # :133
            self.model_keys = None
        self.signals = {bm: {} for bm in self.table.values()} if train else None
        self.contexts = {bm: {} for bm in self.table.values()} if train else None
        self.stdout = None      # where the exit paths' lines go (None: sys.stdout; a stream that will be replayed by the one-table path: a sink)
        self.host_scored = {}   # record -> probability, for the records the host had to score itself (edge contexts)
        self.blobs = []         # emitted rows as text (bytes), in order
        self.num_observations = 0
        self.pos_set, self.multi, self.w_skips, self.skipped = set(), set(), set(), set()
        self._n_pos = self._n_multi = self._n_wskips = self._n_skipped = self._kept_pos = None    # set by the vectorised counters

    # ---- output ----
    def write_to(self, sink):
        """The rows to sink(bytes-like), piece by piece as they were made (no joined copy) -> bytes written."""
        n = 0
        for b in self.blobs:
            if len(b):
                n += len(b)
                sink(b.view if isinstance(b, (_lib.LibBuffer, _lib.RowText)) else b)
            if isinstance(b, _lib.RowText):
                b.release()                                    # (the pinned block goes back to the context)
        return n

    def text(self, max_rows=None):
        """The rows as bytes; max_rows: only the first that many (the reference's 5000-row batches on an exit)."""
        blob = b''.join(b.view if isinstance(b, (_lib.LibBuffer, _lib.RowText)) else b for b in self.blobs)
        if max_rows is None:
            return blob
        return b''.join(blob.splitlines(True)[:max_rows])

    @property
    def rows(self):
        return [line.split('\t') for line in self.text().decode('utf-8', 'surrogateescape').splitlines()]

    def counters(self):
        if self._n_pos is None and self._kept_pos is None and getattr(self, '_counted_natively', False):
            n = self._rec.n
            self._kept_pos = self._site_pos[:n][(self._info[:n] & _I.I_TOO_MANY) == 0]
        if self._n_pos is None and self._kept_pos is not None:
            self._n_pos = len(distinct_positions(self._kept_pos))
        n_pos = len(self.pos_set) if self._n_pos is None else self._n_pos
        n_multi = len(self.multi) if self._n_multi is None else self._n_multi
        n_wskips = len(self.w_skips) if self._n_wskips is None else self._n_wskips
        n_skipped = len(self.skipped) if self._n_skipped is None else self._n_skipped
        return ['thread finished processing...:', '%d observations' % self.num_observations,
                '%d positions' % n_pos, '%d regions with multiple methylated bases' % n_multi,
                '%d observations with skips included' % n_wskips,
                '%d observations with too many skips' % n_skipped]

    def _bind(self, rec):
        n = rec.n
        self._rec = rec
        self._lazy = None

    # (read where the per-record paths need them: a shard whose rows the native formatter prints and whose counters
    # mc_count_records makes leaves narrow records -- Records.site_pos -- as they arrived)
    @property
    def _info(self):
        return self._rec.info[:self._rec.n]

    @property
    def _site_pos(self):
        return self._rec.site_pos[:self._rec.n]

    @property
    def _seg_of(self):
        return self._rec.site_seg[:self._rec.n]

    def _per_record(self):
        """(slot means [calls, k], row of every record in them or None, segment of every record's closing row): only the
        per-record transcription (_one) needs these -- a streamed predict-mode shard whose rows all come from the native
        formatter leaves the packed slot means (mc_calls_view.feats_lo32) as they arrived."""
        if self._lazy is None:
            rec, k, t, n = self._rec, self.k, self.P.table, self._rec.n
            m = rec.n_calls                   # (a compacted view, mc_wait_records: rows of the calls only, see Records.call_row)
            feats = rec.feats[:m * k].reshape(m, k)
            row = rec.call_row[:n] if rec.call_row is not None else None
            close_seg = np.searchsorted(t.seg_row_begin, rec.close_row[:n], side='right') - 1
            self._lazy = (feats, row, close_seg)
        return self._lazy

    def run(self, rec):
        """Returns None, or the exception (SystemExit / error) the reference would raise at that record."""
        self._bind(rec)
        n = rec.n
        if self.train or n == 0:
            for j in range(n):
                stop = self._one(j)
                if stop is not None:
                    return stop
            return None
        P, t = self.P, self.P.table
        text = getattr(rec, 'row_text', None)
        if text is not None:
            # the rows came with the records, written on the device (mc_rowtext.hip: every record was one the native formatter
            # would have printed -- anything else and the pass comes without text): the counters are all that is left to do
            self.blobs.append(text)
            self.num_observations += text.n_rows
            self._count(n)
            return None
        label_meth = 'm6A' if self.base == 'A' else 'm' + self.base                # :200-204
        fmt = _lib.DiffsFormatter(rec, t, P.ref.device_arrays(), P.ref.names, [str(q) for q in P.qual_obj], self.k,
                                  label_meth, self.base, self.soc, tail_chrom=self.tail_chrom)
        first, done_to, stop_exc = 0, n, None
        while first < n:
            blob, n_rows, stop = fmt.rows(first, n_threads=FORMAT_THREADS[0])
            self.blobs.append(blob)
            self.num_observations += n_rows
            if stop >= n:
                break
            stop_exc = self._one(stop)                   # the record the formatter handed back
            if stop_exc is not None:
                done_to = stop
                break
            first = stop + 1
        self._count(done_to)
        return stop_exc

    def host_prob(self, rec):
        """Probability per record (one row per record), the host-scored ones filled in."""
        r = rec.by_record()
        p = np.array(r.prob[:r.n], dtype=np.float64)
        for j, v in self.host_scored.items():
            p[j] = v
        return p

    def _count(self, n):
        """The four sets of :184-185,:234-239,:247-248 over records [0, n), vectorised (set sizes only).  The sets hold (read,
        site) pairs, and records come in file order: a table whose read names do not repeat has them in strictly ascending
        order of (read id, site) -- every pair is then a new one and a set's size is a count, no sort (a one-base motif: 150 000
        records per shard, four sorts of them were most of what a shard's rows cost)."""
        if n == self._rec.n and n > 0:
            # (one pass in the library, without the interpreter lock -- mc_count_records; the pairs ascend unless read names repeat)
            counts, ascending, _, _ = self._rec.count(n, seg_read=self.P.table.seg_read)
            if ascending:
                self._n_skipped, self._n_wskips, self._n_multi = counts
                self._kept_pos = None
                self._n_pos = None
                self._counted_natively = True
                return
        info = self._info[:n]
        rid = self.P.table.seg_read[self._seg_of[:n]].astype(np.int64)
        key = (rid << 32) | (self._site_pos[:n].astype(np.int64) & 0xFFFFFFFF)
        too = (info & _I.I_TOO_MANY) != 0
        kept = ~too
        if n < 2 or bool((key[1:] > key[:-1]).all()):
            size = np.count_nonzero
        else:
            size = lambda mask: len(np.unique(key[mask]))            # noqa: E731
        self._n_skipped = int(size(too))
        self._n_wskips = int(size(kept & ((info & _I.I_EMPTY_MASK) != 0)))
        self._n_multi = int(size((info & _I.I_MULTI) != 0))
        self._kept_pos = self._site_pos[:n][kept]           # (the distinct positions: counted when somebody asks, counters())
        self._n_pos = None

    def _one(self, j):
        P, k, t = self.P, self.k, self.P.table
        rec = self._rec
        feats, rows_of, close_seg = self._per_record()
        names = t.read_names
        half = int((2 * k - 1) / 2)
        inf = int(self._info[j])
        seg = int(self._seg_of[j])
        rid = int(t.seg_read[seg])
        read, mpos = names[rid], int(self._site_pos[j])
        rev = bool(inf & _I.I_REV)
        if inf & _I.I_TOO_MANY:
            self.skipped.add((read, mpos))                                    # :239
        else:
            empty = inf & _I.I_EMPTY_MASK
            if empty:
                self.w_skips.add((read, mpos))                                # :184-185
            row = j if rows_of is None else int(rows_of[j])
            diffs = [0 if (empty >> i) & 1 else float(feats[row, i]) for i in range(k)]
            qual = P.qual_obj[rid]
            diffs_txt = ','.join(['0' if (empty >> i) & 1 else fmt_float(feats[row, i]) for i in range(k)]
                                 + [str(qual)])
            cseg = int(close_seg[j])
            chrom = self.tail_chrom if cseg >= t.n_seg else P.ref.names[int(t.seg_contig[cseg])]
            last_ref = P.ref.meth[int(t.seg_contig[seg])][1 if rev else 0]
            context = revcomp(last_ref[mpos - k + 1:mpos + k], rev)           # :194 (Python slicing rules)
            line = read + '\t' + str(mpos) + '\t' + context + '\t' + diffs_txt + '\t' + strand(rev)
            centre = int(len(context) / 2)
            if context[centre] == 'M':                                        # IndexError propagates, as there
                try:
                    twobase_model = self.table[context[centre:centre + 2]]
                    if not self.train:
                        mi = self.model_index[twobase_model]                  # KeyError: model[...] :199
                        p1 = rec.prob[row]
                        want = (inf >> _I.I_NEXT_SHIFT) & 0xFF
                        if (inf & _I.I_EDGE) or np.isnan(p1):
                            dev = self.device if self.device is not None else get_device()
                            p1 = dev.mlp_forward(np.array([diffs + [float(qual)]], dtype=np.float64),
                                                 np.array([mi], dtype=np.uint8))[0]
                            self.host_scored[j] = float(p1)
                        elif len(context) > half + 1 and ord(context[half + 1]) != want:
                            raise AssertionError('device and host disagree on the sub-model of %s' % line)
                        if p1 >= 0.5:
                            label = 'm6A' if self.base == 'A' else 'm' + self.base
                        else:
                            label = self.base
                        label = label + '\t' + fmt_float(round2(p1))          # :207
                    else:
                        label = self.pos_label[(chrom, mpos, strand(rev))]    # :210
                        self.signals[twobase_model].setdefault(label, []).append(diffs + [qual])
                        self.contexts[twobase_model].setdefault(label, []).append(context)
                    row = [chrom, read, str(mpos), context, diffs_txt, strand(rev), label]
                    self.blobs.append(('\t'.join(row) + '\n').encode('utf-8', 'surrogateescape'))
                except (IndexError, KeyError) as e:                           # :218-223
                    print(line, '- Index or Key Error', file=self.stdout)
                    print(list(self.model_keys or []), list(self.table.keys()), context[centre:centre + 2], file=self.stdout)
                    print(e, file=self.stdout)
                    return SystemExit(0)
            else:                                                             # :224-228
                print(line, file=self.stdout)
                return SystemExit(0)
            self.num_observations += 1
            self.pos_set.add(mpos)
        if inf & _I.I_MULTI:
            self.multi.add((read, mpos))                                      # :247-248
        return None


def distinct_positions(pos):
    """np.unique of an array of site positions (small non-negative integers: the contig's length bounds them) without
    sorting it: a mark per position."""
    pos = np.asarray(pos)
    if len(pos) == 0:
        return np.zeros(0, dtype=np.int32)
    lo, hi = int(pos.min()), int(pos.max())
    if lo < 0 or hi - lo > (1 << 28):
        return np.unique(pos)
    seen = np.zeros(hi - lo + 1, dtype=bool)
    seen[pos - lo] = True
    return (np.flatnonzero(seen) + lo).astype(pos.dtype, copy=False)


def cut_names(table, rec):
    """What a cut of the file at a read start can change is `last_read` (extract_contexts.py:161-174): a read whose name equals
    the name of the LAST READ THAT HAD A SITE ROW is tested on `event_idx > first_read_ind` instead of on its k-mers.  A table
    knows that for its own reads (name blocks that repeat: the literal path); across a cut it can only matter for the reads of
    the piece behind the cut up to and including its first read with a site row, against the reads of the piece in front of it
    from its last read with a site row on.  A read with a flush record has a site row, so the reads up to the first one with
    a record (`head`) and the reads from the last one with a record on (`tail`) cover both -- a name that comes back anywhere
    else, gigabytes later, changes nothing.  -> (head names, tail names, the table has records)"""
    names, seg_read = table.read_names, table.seg_read
    n = int(rec.n)
    if n == 0:
        every = set(names[int(r)] for r in seg_read)
        return every, every, False
    first_seg, last_seg = rec.end_segments()
    return (set(names[int(r)] for r in seg_read[:first_seg + 1]), set(names[int(r)] for r in seg_read[last_seg:]), True)


FORMAT_THREADS = [int(__import__('os').environ.get('MCALLER_FORMAT_THREADS', '0'))]     # threads of the native row formatter (0: every core this process may use)


def head_contig(P, qual_thresh):
    """Contig id of the first row of P.table that passes the filters (:167-168), or None: the row that closes the last
    window of the table before it (R6) and supplies that record's chrom column (R8)."""
    t = P.table
    for seg in range(t.n_seg):
        if P.qual[t.seg_read[seg]] < qual_thresh:
            continue
        r0, r1 = int(t.seg_row_begin[seg]), int(t.seg_row_begin[seg + 1])
        if ((t.flags[r0:r1] & _lib.F_MODEL_N) == 0).any():
            return int(t.seg_contig[seg])
    return None
