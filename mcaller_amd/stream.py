"""Shards: a whole file (or one GPU's byte range of it) streamed through the device, the rows of every shard made by rows.py.

Three owners, each with a close() that is safe after any failure: `ShardFeed` (the text on its way to the device and the table
slots no pass has taken yet), `PassQueue` (the passes in flight) and `RowOutput` (the helpers that turn records into rows and
fold every shard into the `StreamResult`).  `stream_features` sets them up, runs the shard loop and closes them in one place.
"""
import contextlib
import functools
import io
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .device import get_device
from .refmark import MarkedReference
from .rows import Finisher, Prepared, base_models, cut_names, head_contig, prepare, prepare_table, submodel_setup

STREAM_SHARD_BYTES = 128 << 20      # eventalign text per shard of a streamed file (~10^6 rows)
STREAM_SHARD_MIN_BYTES = 8 << 20    # ... of a short range, at least (a shard costs the main thread half a millisecond whatever its size)
STREAM_MIN_SHARDS = 24              # ... which is cut into at least this many (shard_schedule)
STREAM_SHARD_MAX_BYTES = 2 << 30    # a shard beyond this (the cuts are at read starts: one giant read) sends the file to the one-table path


def shard_schedule(lo, hi):
    """Where a streamed byte range is cut into shards (offsets, to be moved to read starts): shards of STREAM_SHARD_BYTES, but a
    short range -- the piece of one GPU of a sharded run -- in at least STREAM_MIN_SHARDS of them (ten shards fill and drain a
    six-deep pipeline for a third of their time), and the first three shards an eighth, a quarter, half of that: nothing happens on
    the GPU before the first shard's text has been read and sent, and the last two half and a quarter: what is left to do when
    the last text has arrived is one shard's parse, pass, copy-out and rows."""
    total = hi - lo
    full = int(min(STREAM_SHARD_BYTES, max(STREAM_SHARD_MIN_BYTES, total // STREAM_MIN_SHARDS)))
    if total < 2 * full:
        return [lo + total // 2] if total >= 2 * STREAM_SHARD_MIN_BYTES else []
    head, tail = [full // 8, full // 4, full // 2], [full // 2, full // 4]
    if total < 4 * full:
        head, tail = [], []
    body = total - sum(head) - sum(tail)
    n_body = max(1, int(round(body / float(full))))
    sizes = head + [body // n_body] * n_body + tail
    offs, at = [], lo
    for sz in sizes[:-1]:
        at += sz
        offs.append(at)
    return offs


class _Unstreamable(Exception):
    """The file needs the one-table path (an exit path of the reference, a read name in two shards, ...)."""


class StreamResult(object):
    """What stream_features hands back (the rows themselves went to the sink, shard after shard)."""

    def __init__(self, ref=None, train_keys=None):
        self.ref = ref                  # the MarkedReference the shards shared
        self.counters, self.messages, self.names = [], [], set()
        self.n_rows = self.n_bytes = self.n_obs = self.n_multi = self.n_wskips = self.n_skipped = 0
        self.positions = np.zeros(0, dtype=np.int32)
        self.signals = {key: {} for key in train_keys} if train_keys is not None else None     # (train mode: the reference's dicts)
        self.contexts = {key: {} for key in train_keys} if train_keys is not None else None
        # what crosses a cut of the file in front of / behind this stream (see cut_names): names up to the first read with a
        # flush record, names from the last such read on, whether any read had one
        self.head_names, self.tail_names, self.had_records = set(), set(), False


class Clock(object):
    """What a stream measured of itself (MCALLER_TIMING), summed per key into the plain dict `d` (stream_features.last_clock)."""

    def __init__(self, n_shards, overlap):
        # (hand_out, split: GPU + copy-out waited for | rows formatted | sink; format_threads 0: the main thread formats;
        # events, MCALLER_TIMING=2: when the main thread did what)
        self.d = dict(wait_parser=0.0, hand_out=0.0, enqueue=0.0, parse=0.0, shards=n_shards, wait_records=0.0, format=0.0,
                      write=0.0, out_bytes=0, records=0, device_parsed=0, device_rows=0, overlapped=bool(overlap),
                      format_threads=2 if overlap else 0, events=[])
        self.t_zero = time.perf_counter()

    def add(self, key, n):
        self.d[key] = self.d.get(key, 0) + n

    @contextlib.contextmanager
    def timed(self, key):
        t = time.perf_counter()
        try:
            yield
        finally:
            self.add(key, time.perf_counter() - t)

    def mark(self, what):
        self.d['events'].append((time.perf_counter() - self.t_zero, what))


def _quietly(fn, *a):
    """A step of the teardown: what it raises must not replace what stopped the stream, nor keep the next step from running."""
    try:
        fn(*a)
    except Exception:                                          # noqa
        pass


class ShardFeed(object):
    """The shards on their way to the main thread, in file order.  Two reader / parser threads take them in turn (the native calls
    spread a shard over all cores, but opening, cutting and stitching are serial: two shards in the works hide that); at most
    three shards ahead of the GPU.  The text is parsed on the GPU (mc_ctx_parse_*: the host threads only move the bytes into
    pinned memory -- on a box whose CPU time is rationed the parse is what a file costs) unless MCALLER_HOST_PARSER is set; a
    shard the device parser declines (a number form that needs strtod, ...) goes through the host parser.
    Owns the reader pool, `ahead`, `parsing`, the piece cursor, the marking thread and every table slot no pass has taken yet."""

    def __init__(self, dev, ref, passes, clock, tsv_input, pieces, on_device, mark_all, read2qual, host_parse):
        self.dev, self.ref, self.passes, self.clock = dev, ref, passes, clock
        self.tsv_input, self.pieces, self.on_device, self.mark_all = tsv_input, pieces, on_device, mark_all
        self.read2qual, self.host_parse = read2qual, host_parse     # host_parse(lo, hi) -> Prepared, through the host parser
        self.pool = ThreadPoolExecutor(max_workers=2)
        self.ahead = []                 # (future, piece) of the shards being read / parsed by the host threads, in file order
        self.parsing = []               # (slot, text, piece) of the shards the device is parsing, in file order
        self.lent = []                  # tables in a slot, handed to the main thread: the feed's until a pass takes them or give_back
        self.held = None                # a shard the host parser had to take (too long), until the shards in front of it have gone
        self.cursor = 0                 # the next piece to be read
        self.rows_cap = 0
        self.mark_thread = None

    def reserve_slots(self):
        if not self.on_device:
            return
        biggest = max(b - a for a, b in self.pieces)
        if biggest > STREAM_SHARD_MAX_BYTES:                   # (one giant read: twelve slots of that size are not worth reserving)
            raise _Unstreamable('a shard of %d bytes' % biggest)
        self.rows_cap = biggest // 48 + 65536
        try:
            self.dev.reserve_tables(self.rows_cap, self.rows_cap // 16, self.rows_cap // 16)
        except _lib.McError as e:
            raise _Unstreamable('the table slots cannot be reserved: %s' % e)

    def _read(self, lo_i, hi_i):
        with self.clock.timed('parse'):
            if self.on_device and hi_i - lo_i < (1 << 32) - 64:    # (mc_ctx_parse_begin: at most 4 GB of text per shard)
                return _lib.TextBlock(self.tsv_input, lo_i, hi_i)
            return self.host_parse(lo_i, hi_i)

    def fill_ahead(self):
        """Keeps three shards ahead of the GPU with the reader threads (a held shard is one of them)."""
        while self.cursor < len(self.pieces) and len(self.ahead) + (self.held is not None) < 3:
            piece = self.pieces[self.cursor]
            self.ahead.append((self.pool.submit(self._read, *piece), piece))
            self.cursor += 1

    def _mark_first_contig(self):
        """The first contig of the file is marked while the first shards are read and sent (marking E. coli takes 14 ms; the main
        thread would do it when the first table comes back, with the GPU waiting).  An exit path of the marking is left to
        the main thread: it marks again and meets it there."""
        ref = self.ref
        try:
            with open(self.tsv_input, 'rb') as fh:
                fh.seek(self.pieces[0][0])
                for line in fh.read(1 << 16).splitlines():
                    tok = line.split()
                    if len(tok) >= 12 and tok[0].decode('utf-8', 'surrogateescape') in ref.names:
                        cid = ref.names.index(tok[0].decode('utf-8', 'surrogateescape'))
                        ref.mark(cid)                          # (ref.quiet: nothing is printed from here)
                        ref.device_arrays()                    # (cached: the main thread's set_reference finds them made)
                        return
        except BaseException:                                  # noqa
            pass

    def top_up(self):
        """Text of the shards ahead on its way to the device (back to back over the link; 12 table slots), up to six shards --
        four until the reference masks are there: they travel over the same link and the first pass waits for them.  Called
        wherever the main thread is about to wait.  A shard the host parser had to take (too long) is `held` from here on: file
        order, the shards in front of it come first and nothing behind it is begun (next() hands it out when it is its turn)."""
        while self.held is None and self.ahead and len(self.parsing) < (6 if self.passes.marked >= 0 else 4):
            fut, piece = self.ahead.pop(0)
            text = fut.result()
            if not isinstance(text, _lib.TextBlock):           # a shard too long for the device parser: parsed by the host already
                self.held = text
                break
            self.clock.mark('text ready')
            self.parsing.append((self.needs_a_slot(self.dev.parse_begin, text, self.ref.names, self.rows_cap), text, piece))
            self.clock.mark('parse_begin done')
            # (started when three shards of text are on their way: what is left of the marking under the interpreter lock -- making
            # Python strings of 2 x 4.6 MB -- would hold up the reader threads at the very start)
            if self.mark_thread is None and not self.mark_all and (len(self.parsing) >= 3 or self.cursor >= len(self.pieces)):
                self.mark_thread = threading.Thread(target=self._mark_first_contig, daemon=True)
                self.mark_thread.start()
            self.fill_ahead()

    def needs_a_slot(self, fn, *a):
        """A call that takes a table slot (mc_ctx_parse_begin, mc_ctx_upload_table_async): with every slot taken the oldest pass is
        handed out first; whatever else the streaming machinery declines sends the file to the one-table path."""
        while True:
            try:
                return fn(*a)
            except _lib.McError as e:
                if e.code == _lib.E_NO_FREE_SLOT and self.passes.in_flight:
                    self.passes.hand_out()
                    continue
                raise _Unstreamable('the streaming machinery declined: %s' % e)

    def next(self):
        """The next shard in file order (None behind the last); keeps the parser threads (and the device parser) busy."""
        self.fill_ahead()
        if not self.on_device:
            return self.ahead.pop(0)[0].result() if self.ahead else None
        self.top_up()
        if not self.parsing:
            P_held, self.held = self.held, None                # (its turn has come; None behind the last shard)
            return P_held
        slot, text, piece = self.parsing[0]
        self.clock.mark('parse_end ...')
        try:
            table = self.dev.parse_end(slot, text)
        except _lib.McError as e:                              # (the slot is still in `parsing`: close() gives it back)
            raise _Unstreamable('the device parser failed: %s' % e)
        del self.parsing[0]
        self.clock.mark('parse_end done')
        if table is None:                                      # declined: the host parser takes the shard
            return self.host_parse(*piece)
        self.clock.add('device_parsed', 1)
        self.lent = [t for t in self.lent if t.device_slot is not None] + [table]
        self.top_up()                                          # (the marking of the first contig may be waited for next)
        P_new = prepare_table(Prepared(), table, self.ref, self.read2qual, quiet=True)
        self.clock.mark('prepared')
        return P_new

    def give_back(self, table):
        """A table the device parser has put into a slot and that no pass will scan: the slot is free again."""
        slot = getattr(table, 'device_slot', None)
        if slot is not None:
            self.dev.parse_abandon(slot)
            table.device_slot = None

    def close(self):
        """Nothing more is read, and every slot no pass has taken is free again (none is left when the stream came to its end)."""
        self.cursor = len(self.pieces)
        for fut, _ in self.ahead:
            fut.cancel()
        for slot, _, _ in self.parsing:                        # tables the device parser was filling: their slots go back
            _quietly(self.dev.parse_abandon, slot)
        for table in reversed(self.lent):                      # ... and the tables the shard loop held when it was stopped
            _quietly(self.give_back, table)
        del self.parsing[:], self.lent[:]
        if self.mark_thread is not None:
            self.mark_thread.join()
        self.pool.shutdown(wait=True)


class PassQueue(object):
    """The passes enqueued and not yet handed out, at most two, with what they scan besides the table: the reference masks and
    the row writer's switch.  in_flight: (P, tail name, rows of the shards before it), oldest first."""

    def __init__(self, dev, ref, rows, clock, k, skip_thresh, qual_thresh, base, train, on_device, device_rows):
        self.dev, self.ref, self.rows, self.clock = dev, ref, rows, clock
        self.k, self.skip_thresh, self.qual_thresh, self.train = k, skip_thresh, qual_thresh, train
        self.labels = ('m6A' if base == 'A' else 'm' + base, base)                # :200-204
        self.on_device, self.device_rows = on_device, device_rows
        self.feed = None                # (the ShardFeed, which is made with this queue: each calls the other)
        self.in_flight = []
        self.masks_on_device = False    # the site masks of every contig were made on the GPU (masks_from_motif)
        self.marked = -1                # contigs whose masks were uploaded last (>= 0: the reference masks are on the device)
        self.row_text_on = False

    def start_row_text(self):
        """The rows themselves are written on the GPU, behind the records they are made from (mc_rowtext.hip), when the
        shard's table is one the device parser made: what is left for the helpers is the counters and the write.
        MCALLER_DEVICE_ROWS=0: the host formatter throughout."""
        if self.device_rows:
            self.dev.row_text(True, *self.labels, first=True)  # (the blocks of a stream that failed are free again)
            self.row_text_on = True

    def masks_from_motif(self):
        """Motif mode: the site masks of every contig are made on the GPU, from the raw bases, before the first text is on its way
        (mc_ctx_set_reference_motif) -- the marked strings the rows' contexts are sliced from are made by a thread meanwhile and
        are not waited for by the passes.  (Not for motifs that can overlap themselves, positions mode, very long references:
        then the masks come from the host's marking, contig by contig as they appear.)"""
        dev_motif = self.ref.motif_for_the_device() if self.on_device else None
        dev_iupac = self.ref.iupac_for_the_device() if self.on_device else None       # (a --motifs spec: mc_ctx_set_reference_iupac)
        if (dev_motif is None and dev_iupac is None) or sum(len(seq) for _, seq in self.ref.records) > (256 << 20):
            return
        if dev_iupac is not None:
            self.dev.set_reference_iupac(self.ref.raw_arrays(), dev_iupac)
        else:
            self.dev.set_reference_motif(self.ref.raw_arrays(), *dev_motif)
        self.masks_on_device = True
        self.marked = 0

    def enqueue(self, P, tail_id, rows_before):
        while len(self.in_flight) >= 2:
            self.hand_out()
        with self.clock.timed('enqueue'):
            self.clock.mark('enqueue ...')
            self._upload_and_run(P, tail_id)
            self.clock.mark('enqueued')
        self.in_flight.append((P, self.ref.names[tail_id] if tail_id >= 0 else None, rows_before))
        if self.device_rows and len(self.in_flight) >= 2:
            self.dev.wait_begin()                              # (the oldest pass's copy-out and row writer start now, not when it is waited for)

    def _upload_and_run(self, P, tail_id):
        dev = self.dev
        n_marked = len(self.ref.meth)                          # (the parser thread marks contigs as they first appear)
        if not self.masks_on_device and n_marked != self.marked:      # a contig marked since the last upload: new masks
            self.drain()
            if self.on_device:
                self.feed.top_up()                             # (the link stays busy while the masks are made ready)
            dev.set_reference(self.ref.device_arrays())
            self.marked = n_marked
        self.feed.needs_a_slot(dev.upload_table_async, P.table, P.qual)
        if self.device_rows:
            # (str(quality) on the device is repr of the double: for what read_qual / the FASTQ reader return, floats)
            dev.row_text(all(isinstance(q, float) for q in P.qual_obj), *self.labels)
        dev.run_async(self.k, self.skip_thresh, self.qual_thresh, tail_contig=tail_id, score=not self.train)

    def hand_out(self):
        with self.clock.timed('hand_out'):
            P, tail, rows_before = self.in_flight.pop(0)
            self.clock.mark('wait ...')
            with self.clock.timed('wait_records'):
                rec = self.dev.wait()
            self.clock.mark('records here')
            self.rows.take(P, tail, rows_before, rec)

    def drain(self):
        while self.in_flight:
            self.hand_out()

    def close(self):
        """Nothing may stay in flight on the shared device: what is left is waited for and dropped."""
        while self.in_flight:
            self.in_flight.pop(0)
            _quietly(self.dev.wait)
        if self.row_text_on:
            _quietly(self.dev.row_text, False)


class RowOutput(object):
    """The rows of a shard are formatted by helper threads and appended by another while the main thread goes on to the next shard (its
    table, its passes, the wait for its records): a one-base motif writes 1.3 GB of rows per 10^8 events, and formatter + write were
    two thirds of what the main thread did.  TWO formatting helpers take the shards in turn: what a shard costs there is the native
    formatter on all host cores (2.5 ms per 10^6 rows of a one-base motif, one call at a time) and 1.5 ms of interpreter around it
    (the counters, the names at the cuts, the marks) -- the one's interpreter part runs beside the other's native part.  What depends
    on the order of the shards (names across the cuts, the rows handed to the writer, the totals) is done by every shard in its turn.
    Not in train mode (the per-record transcription holds the interpreter lock) and not when every shard's records are reduced on
    the device (on_shard needs what the formatter found): `overlap` is off then, and the main thread does it all.  The helpers are
    at most two shards behind: the records they read stay where they are until six more passes have been enqueued.
    Owns the two pools, `pending`, `writes`, the chain of turn events and `failed`; folds every shard into the StreamResult."""

    def __init__(self, out, finisher, sink, on_shard, overlap, clock):
        self.out, self.finisher, self.sink, self.on_shard, self.overlap, self.clock = out, finisher, sink, on_shard, overlap, clock
        self.fmt_pool = ThreadPoolExecutor(max_workers=2) if overlap else None
        self.write_pool = ThreadPoolExecutor(max_workers=1) if overlap else None     # (... and one more appends them: in order, one shard behind)
        self.pending, self.writes = [], []      # the helpers' jobs in flight (futures), if any
        self.turn = None                # the event the shard handed out last sets when its part in order is done
        self.failed = False             # a shard met an exit path or a name on both sides of a cut: the shards behind it write nothing
        self.positions = np.zeros(1 << 16, dtype=bool)         # positions[p]: a call at site position p has been seen

    def wait_for(self, leave=0):
        while len(self.pending) > leave:
            self.pending.pop(0).result()                       # (its exception, if it met an exit path, is raised here)
        if not leave:
            while self.writes:
                self.writes.pop(0).result()

    def take(self, P, tail, rows_before, rec):
        if not self.overlap:
            return self._finish(P, tail, rows_before, rec, None)
        with self.clock.timed('wait_formatter'):
            self.wait_for(leave=1)                             # (the shard before the last: done, or its exit path raised)
        before, mine = self.turn, threading.Event()
        self.turn = mine
        self.pending.append(self.fmt_pool.submit(self._finish_in_turn, P, tail, rows_before, rec, before, mine))

    def _finish_in_turn(self, P, tail, rows_before, rec, before, mine):
        try:
            self._finish(P, tail, rows_before, rec, before)
        except BaseException:
            self.failed = True
            raise
        finally:
            mine.set()

    def _finish(self, P, tail, rows_before, rec, before):
        out = self.out
        t_f = time.perf_counter()
        fin = self.finisher(P, tail_chrom=tail)
        fin.stdout = io.StringIO()                             # (its exit paths print; the one-table path will)
        stop = fin.run(rec)
        ran = time.perf_counter() - t_f
        if before is not None:
            before.wait()                                      # ---- from here on: in the order of the shards ----
            if self.failed:
                return
        with self.clock.timed('format'):                       # (the wait for the turn is not formatting)
            self.clock.add('format', ran)
            if stop is not None:
                raise _Unstreamable('an exit path of the reference')
            # `last_read` across the cut in front of this shard (cut_names): a name on both sides of it sends the file to the one-table path
            head_n, tail_n, has_rec = cut_names(P.table, rec)
            if head_n & out.tail_names:
                raise _Unstreamable('a read name on both sides of a cut between two shards')
            if not out.had_records:
                out.head_names |= head_n
            out.tail_names = tail_n if has_rec else (out.tail_names | tail_n)
            out.had_records = out.had_records or has_rec
        if self.overlap:
            while len(self.writes) > 1:                        # (at most two shards' rows wait to be written)
                self.writes.pop(0).result()
            self.writes.append(self.write_pool.submit(self._write, fin))
        else:
            self._write(fin)
        self._fold(fin, rec)
        if self.on_shard is not None:
            self.on_shard(P, rec, fin, tail, rows_before)

    def _write(self, fin):
        with self.clock.timed('write'):
            n_out = fin.write_to(self.sink)
        self.clock.add('out_bytes', n_out)
        self.out.n_bytes += n_out

    def _fold(self, fin, rec):
        out, n = self.out, rec.n
        self.clock.add('records', int(n))
        self.clock.add('device_rows', 1 if getattr(rec, 'row_text', None) is not None else 0)
        if n:
            # the distinct positions of the file: a mark per position, counted at the end (mc_count_records: one pass in the library)
            _, _, lo_pos, top = rec.count(n, pos_marks=self.positions)
            if lo_pos < 0:
                raise _Unstreamable('a negative site position')
            if top > len(self.positions):
                grow = max(top, 2 * len(self.positions)) - len(self.positions)
                self.positions = np.concatenate([self.positions, np.zeros(grow, dtype=bool)])
                rec.count(n, pos_marks=self.positions)
        # (train mode goes record by record: its sets count; else the vectorised counters have the sizes)
        out.n_obs += fin.num_observations
        out.n_multi += len(fin.multi) if fin._n_multi is None else fin._n_multi
        out.n_wskips += len(fin.w_skips) if fin._n_wskips is None else fin._n_wskips
        out.n_skipped += len(fin.skipped) if fin._n_skipped is None else fin._n_skipped
        for mine, theirs in ((out.signals, fin.signals), (out.contexts, fin.contexts)):
            for key, by_label in (theirs or {}).items():
                for label, rows in by_label.items():
                    mine[key].setdefault(label, []).extend(rows)

    def totals(self, n_rows):
        out = self.out
        out.n_rows = n_rows
        out.positions = np.flatnonzero(self.positions).astype(np.int32)
        out.counters = ['thread finished processing...:', '%d observations' % out.n_obs, '%d positions' % len(out.positions),
                        '%d regions with multiple methylated bases' % out.n_multi,
                        '%d observations with skips included' % out.n_wskips,
                        '%d observations with too many skips' % out.n_skipped]

    def close(self):
        """The helpers must be done with the records before anything they read is torn down (what they raised has been raised by
        wait_for, or came after what stopped the stream)."""
        for fut in self.pending + self.writes:
            try:
                fut.result()
            except BaseException:                              # noqa
                pass
        del self.pending[:], self.writes[:]
        if self.overlap:
            self.fmt_pool.shutdown(wait=True)
            self.write_pool.shutdown(wait=True)


def _cut(tsv_input, endline, byte_range, n_shards, min_shards):
    """The byte ranges of the shards, in file order; []: the range of a GPU of a sharded run that holds no read."""
    if byte_range is None:
        lo, hi = _lib.eventalign_consumed_range(tsv_input, 0, endline)
    else:
        lo, hi = byte_range
    if n_shards is None:
        want = shard_schedule(lo, hi)
        if len(want) + 1 < min_shards:
            raise _Unstreamable('one shard')
        cuts = _lib.eventalign_read_cuts_at(tsv_input, want, lo, hi)
    else:
        if n_shards < min_shards:
            raise _Unstreamable('one shard')
        cuts = _lib.eventalign_read_cuts(tsv_input, n_shards, lo, hi)
    pieces = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1) if cuts[i + 1] > cuts[i]]
    if pieces or byte_range is None:   # (a range without a read, fewer reads than GPUs, is a finished piece: not a reason to send the whole file to one GPU)
        if len(pieces) < min_shards:
            raise _Unstreamable('one shard')
    return pieces


def _shard_loop(feed, passes, rows, out, ref, clock, qual_thresh, on_head, tail_of_last):
    """Every shard in file order: a shard is enqueued when the one behind it is known (its first unfiltered row closes the last
    window of the shard in front of it, R6/R8).  -> table rows seen."""
    P = prev = None
    head_told = False
    rows_seen, prev_rows_before = 0, 0
    while True:
        with clock.timed('wait_parser'):
            P = feed.next()
        if P is not None:
            if P.fatal is not None:
                raise _Unstreamable('an exit path of the reference')
            out.names.update(P.table.read_names)                       # (what crosses a cut is looked at when the shard's records are here)
            out.messages.extend(P.messages)
            rows_before = rows_seen
            rows_seen += P.table.n_rows
            if P.table.n_rows == 0:
                feed.give_back(P.table)
                continue
            head = head_contig(P, qual_thresh)
            if head is None:
                feed.give_back(P.table)
                continue                                   # no row passes the filters (:167-168): the loop never sees this shard
            if not head_told and on_head is not None:
                on_head(ref.names[head])
            head_told = True
        if prev is not None:
            if P is not None:
                tail_id = head
            else:                                          # the range's last shard: what follows the range closes its last window
                tail_name = tail_of_last() if tail_of_last is not None else None
                tail_id = ref.names.index(tail_name) if tail_name is not None else -1
            passes.enqueue(prev, tail_id, prev_rows_before)
        prev = P
        if P is None:
            break
        prev_rows_before = rows_before
    if not head_told and on_head is not None:
        on_head(None)
    passes.drain()
    rows.wait_for()
    return rows_seen


def stream_features(tsv_input, fasta_input, read2qual, k, skip_thresh, qual_thresh, modelset, endline, base, motif,
                    positions_list, n_shards=None, device=None, sink=None, byte_range=None, tail_of_last=None, on_head=None,
                    on_shard=None, mark_all=False, min_shards=2, train=False, pos_label=None):
    """A whole file (or the byte range of one GPU of a sharded run), as the reference's batch loop (:140-148) streams it -- here
    in shards cut at read starts (a window never spans two reads, :179,:242): two threads read the shards' text into pinned
    memory, the main thread keeps the text of up to six shards on its way to the GPU, where it is parsed (mc_ctx_parse_begin /
    _end / _finish; a shard the device parser declines, or every shard with MCALLER_HOST_PARSER, goes through the host parser
    and mc_ctx_upload_table_async), two passes in flight (mc_extract_features_async), and formats the rows of the shards that
    come back; reading, H2D, parsing, kernels, D2H and formatting overlap.  The rows of a shard go to `sink(bytes)` as soon as
    they exist, in file order (the reference appends every 5000 observations, :230-232): memory is bounded by the shards in
    flight, whatever the file's size.

    byte_range: (lo, hi), both at first lines of reads, instead of what the reference's loop consumes of (0, endline);
    tail_of_last(): called when the last shard is about to be enqueued -> name of the contig of the first unfiltered row
    BEHIND the range (it closes the range's last window, R6/R8), None: end of file; on_head(name | None): called once, as soon as
    the contig of the range's own first unfiltered row is known (what closes the range in front of it);
    on_shard(P, rec, fin, tail name, rows of the shards before): every shard's records when they have been handed out (the
    per-site reduction of a --bed run); mark_all: every contig is marked before the first pass (one site numbering for all the
    GPUs of a run); train: features only, the reference's train dicts are collected (pos_label) and returned.
    -> StreamResult, or raises _Unstreamable (an exit path of the reference, a read name on both sides of a cut -- cut_names():
    whoever called decides what becomes of the rows the sink has seen).  sink() is handed bytes-like objects that are valid
    during the call only."""
    t_enter = time.perf_counter()
    dev = device if device is not None else get_device()
    env = os.environ                   # (read per call: the switches may change between two streams of one process)
    if n_shards is None:
        n_shards = int(env.get('MCALLER_STREAM_SHARDS', '0')) or None
    on_device = not env.get('MCALLER_HOST_PARSER')
    overlap = not train and on_shard is None and not env.get('MCALLER_NO_OVERLAP')
    device_rows = on_device and not train and env.get('MCALLER_DEVICE_ROWS', '1') != '0'
    pieces = _cut(tsv_input, endline, byte_range, n_shards, min_shards)
    if not pieces:
        if on_head is not None:
            on_head(None)
        stream_features.last_clock = dict(shards=0)
        return StreamResult()
    ref = MarkedReference(fasta_input, base, motif, positions_list)
    ref.quiet = True                   # (an exit path sends the file to the one-table path, which prints)
    if not train:
        _, weights, _, soc = submodel_setup(modelset, base)
        dev.set_classifier(weights, soc)               # (MLP or forest: either runs behind the emit of a pipelined pass)
    out = StreamResult(ref, base_models(base, False).values() if train else None)     # :133
    L = _lib.lib()
    L.mc_host_pool_config(1, -1)                           # the parser's tables live in pinned memory, recycled
    clock = Clock(len(pieces), overlap)
    finisher = functools.partial(Finisher, k=k, base=base, train=train, modelset=modelset, pos_label=pos_label, device=dev)
    rows = RowOutput(out, finisher, sink, on_shard, overlap, clock)
    passes = PassQueue(dev, ref, rows, clock, k, skip_thresh, qual_thresh, base, train, on_device, device_rows)
    host_parse = functools.partial(prepare, tsv_input, None, read2qual, base=base, motif=motif, positions_list=positions_list,
                                   exact_range=True, ref=ref, quiet=True)
    passes.feed = feed = ShardFeed(dev, ref, passes, clock, tsv_input, pieces, on_device, mark_all, read2qual, host_parse)
    done = False
    try:
        feed.reserve_slots()
        clock.t_zero = time.perf_counter()
        passes.start_row_text()
        feed.fill_ahead()                                      # (the first shards are read while the masks are made)
        passes.masks_from_motif()
        if mark_all:                                           # (one site numbering for every GPU of the run: all contigs, now)
            for cid in range(len(ref.names)):
                ref.mark(cid)
        clock.d['setup'] = time.perf_counter() - t_enter       # (cuts, FASTA, classifier, table slots, masks: before the first shard is asked for)
        t_loop = time.perf_counter()
        rows_seen = _shard_loop(feed, passes, rows, out, ref, clock, qual_thresh, on_head, tail_of_last)
        done = True
    finally:
        # (whatever stopped the stream: the helpers first, they read the records; then the device, slots before passes)
        rows.close()
        if not done:
            _quietly(dev.sync)
        feed.close()
        passes.close()
        L.mc_host_pool_config(0, -1)
    clock.d['loop'] = time.perf_counter() - t_loop
    rows.totals(rows_seen)
    stream_features.last_clock = clock.d
    return out
