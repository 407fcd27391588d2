/*
 * mcaller_hip.h -- C ABI of libmcaller_hip.so, the MI355X-native replacement for the hot path of
 * al-mcintyre/mCaller:
 *
 *   extract_contexts.py::extract_features   (reference extract_contexts.py:110-303)
 *     - the per-row 6-slot window machine over nanopolish eventalign rows   (:147-291)
 *     - model[key].predict_proba([diffs]) per observation                    (:199)
 *
 * The reference has no FFI: the path sits behind the Python call boundary
 * `extract_features(tsv_input, fasta_input, read2qual, k, skip_thresh, qual_thresh, modelfile,
 * classifier, startline, endline, train, pos_label, base, motif, positions_list)`
 * (extract_contexts.py:110, called at mCaller.py:53,58,60).  A maintainer of the reference binds the
 * entry points below with ctypes; mcaller_amd/extract_contexts.py is that
 * binding, with the reference's signature.
 *
 * Conventions: every function returns 0 on success, <0 on error (text via mc_last_error(), thread
 * local; MC_E_NO_FREE_SLOT is the one code a caller acts on: hand out the oldest pass and try again).  Plain pointers and sizes only; no exceptions or callbacks cross the ABI.  Host buffers are
 * caller-allocated and never retained after the call returns.  One mc_ctx per GPU; calls on a ctx
 * are serialised by the caller (one process per GPU).
 *
 * This file is also read as text by the Python binding (mcaller_amd/_abi.py), which takes every struct, integer constant and
 * prototype from it and stops on what it does not understand.  So it stays in a small subset of C: plain declarations, one
 * statement each; char, int, float, double and the fixed-width <stdint.h> types; `typedef struct x { ... } x;` whose fields are
 * such scalars, pointers, earlier structs of this file and arrays of them; array sizes and `#define MC_...` values that are
 * integer expressions over literals and earlier defines; opaque handles as `typedef struct x x;`.  No unions, bit fields,
 * enums, function pointers, function-like macros or other typedefs.
 */
#ifndef MCALLER_HIP_H
#define MCALLER_HIP_H

/* mc_ctx_upload_table_async / mc_ctx_parse_begin: every table slot is taken by a pass in flight (or by the records handed out
 * last).  Not a failure of the stream: mc_wait_records frees a slot. */
#define MC_E_NO_FREE_SLOT (-16)

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_MAX_K 8            /* -n/--num_variables supported: 1..8 (reference default 6, mCaller.py:131) */

/* ---- columnar event table (one entry per eventalign row the reference's loop would process) ---- */
/* flags column bits */
#define MC_F_KMER_EQ    0x01  /* reference_kmer (col 3) == model_kmer (col 10)      extract_contexts.py:169 */
#define MC_F_MODEL_N    0x02  /* model_kmer == "NNNNNN"                            extract_contexts.py:167 */
#define MC_F_SEG_START  0x04  /* first row of a (read name, contig) segment                          */
#define MC_F_NAME_START 0x08  /* first row of a name block (maximal run of rows with one read name)  */

typedef struct mc_table_view {
    int64_t n_rows;
    const int32_t *pos;        /* col 2: 0-based k-mer start                                  :175 */
    const int32_t *event_model_e4; /* [2*n_rows] per row: col 7 event_level_mean, col 11 model_mean, in units of 1e-4 pA,
                                      interleaved -- the parser writes the pair, and a window's events are one DRAM page :286.
                                      |value| < 10^9 (the kernels take event - model in 32 bits; both parsers refuse a row
                                      beyond that, or hand over the rounded difference and a model of 0) */
    const int32_t *event_idx;  /* col 6                                                   :162,169 */
    const uint8_t *flags;      /* MC_F_*                                                           */
    int32_t n_seg;
    const int64_t *seg_row_begin; /* [n_seg+1] */
    const int32_t *seg_read;      /* [n_seg] read id: equal names <=> equal ids               :161 */
    const int32_t *seg_contig;    /* [n_seg] contig id (index into the reference set)         :154 */
    int32_t n_reads;
    const uint8_t *model_n_bits;  /* [ceil(n_rows / 8)] bit r & 7 of byte r >> 3: (flags[r] & MC_F_MODEL_N) != 0 -- the one bit of the
                                     flag column the scan looks at, 1/8 B/row where the flag bytes are 1 (mc_pack_model_n).  NULL: the
                                     upload calls pack it from `flags` */
    const uint16_t *idx_rel_bits; /* [ceil(n_rows / 8)] one word per unit of eight rows, row r = 8u + e: bit e of word u is
                                     event_idx[r] > event_idx[r-1], bit 8 + e is event_idx[r] < event_idx[r-1] (neither: equal) --
                                     the row before it in the TABLE, whatever block that belongs to; row 0: neither.  All the
                                     first pass's validation asks of the index column, 1/4 B/row where the indices are 4
                                     (mc_pack_idx_rel).  NULL: the upload calls pack it from `event_idx` */
} mc_table_view;
/* The model-N bit column of a flag column: out[r >> 3] bit r & 7 = (flags[r] & MC_F_MODEL_N) != 0, every byte of
 * [0, ceil(n_rows / 8)) written (bits at or beyond n_rows: 0). */
void mc_pack_model_n(const uint8_t *flags, int64_t n_rows, uint8_t *out);
/* The index-relation column of an event-index column (mc_table_view.idx_rel_bits): every word of [0, ceil(n_rows / 8))
 * written (row 0 and the bits at or beyond n_rows: 0). */
void mc_pack_idx_rel(const int32_t *event_idx, int64_t n_rows, uint16_t *out);

/* ---- marked reference: what find_and_methylate builds (extract_contexts.py:60-81), as bitmasks ---- */
typedef struct mc_ref_view {
    int32_t n_contigs;
    const int64_t *contig_len;    /* [n_contigs] */
    const int64_t *seq_off;       /* [n_contigs] byte offset of the contig in seq                    */
    const uint8_t *seq;           /* upper-cased bases, ASCII                                    :80 */
    const int64_t *word_off;      /* [n_contigs] u32-word offset of the contig in mbits_*            */
    const uint32_t *mbits_fwd;    /* bit p set <=> meth_fwd[p]=='M'; >= 2 zero words of padding  :62 */
    const uint32_t *mbits_rev;    /* bit p set <=> meth_rev[p]=='M'                              :63 */
    int64_t n_seq_bytes, n_words;
} mc_ref_view;

/* ---- flush records: one per window the machine closes (extract_contexts.py:179-239) ---- */
/* info bits */
#define MC_I_EMPTY_MASK   0x000000FFu /* bit i: feature i (final order) came from an empty slot -> literal 0 :186 */
#define MC_I_REV          0x00000100u /* strand '-'                                               :216 */
#define MC_I_TOO_MANY     0x00000200u /* num_skips > skip_thresh: counted, not emitted            :239 */
#define MC_I_MULTI        0x00000400u /* the closing row shifted the window with kmer[0]!='M'     :247 */
#define MC_I_EDGE         0x00000800u /* context slice leaves the contig: host decides (Python slicing) */
#define MC_I_NEXT_SHIFT   16          /* bits 16..23: context[k] (ASCII) -> sub-model key   :197 */

typedef struct mc_calls_view {
    int64_t capacity;
    double  *feats;      /* [capacity*k] slot means in the order the reference prints them   :186-188 */
    int32_t *site_pos;   /* mpos                                                                 :216 */
    int32_t *site_seg;   /* segment of the window's last site row -> read name, site contig      :216 */
    int64_t *close_row;  /* row that closed the window (its contig is the chrom column, R8); n_rows if
                            the closing row lies beyond this table (see tail_contig)             :216 */
    uint32_t *info;      /* MC_I_* */
    double  *prob;       /* p(m6A) from the MLP/forest; NaN where not scored                     :199 */
    /* compacted == 0: feats and prob hold one row per record (row j = record j).  compacted != 0 (mc_wait_records): they
     * hold n_call_rows rows, one per record WITHOUT MC_I_TOO_MANY, in record order (the reference only counts the others,
     * :239, nothing is stored for them): the row of record j is the number of records before j without MC_I_TOO_MANY.
     * call_row, if not NULL, holds that number for every record (-1 for a MC_I_TOO_MANY record); mc_wait_records leaves it
     * NULL -- the copy-out over PCIe bounds a pass, a column the host can derive is not sent (mc_calls_expand fills one). */
    int32_t *call_row;
    int64_t n_call_rows;
    /* mc_wait_records on a table of fewer than 2^31 - 1 rows: close_row is NULL and the closing rows are here. */
    int32_t *close_row32;
    int32_t compacted;
    /* mc_wait_records: feats is NULL and the slot means of call row r, slot s, are packed -- a slot mean that is
     * fl(d / 10^4) for a 32-bit integer d (every slot that holds one event is; the host divides again and gets the same
     * double) travels as d in feats_lo32[r*k + s]; one that is not has bit s of feats_wide[r] set, its low 32 bits in
     * feats_lo32[r*k + s] and its high 32 bits in feats_hi32[j], j = the number of wide slots before it in (row, slot)
     * order.  mc_format_diffs reads that layout; mc_calls_expand unpacks it. */
    const int32_t *feats_lo32;
    const uint32_t *feats_hi32;
    const uint8_t *feats_wide;
    int64_t n_wide;
    /* mc_wait_records, "narrow records": site_pos, site_seg, info, close_row and close_row32 are NULL and the four columns travel
     * as 16-bit halves plus a run list (the sparse MLP passes on tables of fewer than 2^31 - 1 rows whose rows the host prints) --
     * close_lo16[j] = close_row & 0xFFFF, pos_lo16[j] = site_pos & 0xFFFF, info_lo16[j] = info & 0xFFFF, info_next[j] = info >> 16
     * (bits 24..31 of info are 0); runs holds n_runs entries of four int32 { first_record, site_seg, close_row >> 16,
     * site_pos >> 16 } (arithmetic shifts), first_record ascending from 0: an entry says the segment and the high halves of
     * every record from first_record up to the next entry's.  Record j starts an entry iff j == 0 or one of the three differs
     * from record j - 1's.  mc_format_diffs and mc_count_records read either layout; mc_records_expand rebuilds the columns. */
    const uint16_t *close_lo16;
    const uint16_t *pos_lo16;
    const uint16_t *info_lo16;
    const uint8_t *info_next;
    const int32_t *runs;
    int64_t n_runs;
    /* mc_wait_records: bytes the pass's records took on their way to the host, in whichever layout (0: not a packed pass) */
    int64_t copy_out_bytes;
} mc_calls_view;

const char *mc_last_error(void);
const char *mc_version(void);
/* Cores this process may run on (sched_getaffinity) -- what the parser, the FASTQ reader and the row formatter size their
 * thread counts by when n_threads <= 0: a worker bound to its GPU's NUMA node starts one thread per core of that node. */
int mc_host_cores(void);
/* The marking of a contig for a motif (extract_contexts.py:33-41,:60-73) without the interpreter lock: upper_out = seq
 * upper-cased (ASCII), fwd_out / rev_out = upper_out with every occurrence of motif_fwd / motif_rev (left to right,
 * non-overlapping, like str.replace) replaced by repl_fwd / repl_rev of the same length; all buffers n bytes. */
int mc_mark_motifs(const char *seq, int64_t n, const char *motif_fwd, const char *repl_fwd, int32_t m_fwd,
                   const char *motif_rev, const char *repl_rev, int32_t m_rev, char *upper_out, char *fwd_out, char *rev_out);

/* ===== degenerate (IUPAC) motifs, several at once (--motifs; the rule: csrc/mc_iupac.h) =====
 * One motif of one strand: letter i as a set over A, C, G, T (bits 1, 2, 4, 8), bit j of `called`: letter j is marked. */
#define MC_IUPAC_MAX_MOTIFS 8
#define MC_IUPAC_MAX_LEN 32
typedef struct mc_iupac_motif {
    int32_t m;                            /* 1 .. MC_IUPAC_MAX_LEN letters */
    uint32_t called;
    uint8_t set[MC_IUPAC_MAX_LEN];
} mc_iupac_motif;
typedef struct mc_iupac_spec {
    int32_t n_motifs, pad;                /* 1 .. MC_IUPAC_MAX_MOTIFS */
    mc_iupac_motif fwd[MC_IUPAC_MAX_MOTIFS];    /* what is looked for on the forward sequence for the '+' strand ...      */
    mc_iupac_motif rev[MC_IUPAC_MAX_MOTIFS];    /* ... and for the '-' strand: the reverse complements, offsets mirrored */
} mc_iupac_spec;
/* Appends a motif (upper-case IUPAC letters; bit j of called: letter j is marked) to the spec, both strands' tables; a spec
 * starts zero-filled. */
int mc_iupac_spec_add(mc_iupac_spec *spec, const char *motif, int32_t m, uint32_t called);
/* The marking of a contig for a spec, sequentially and without the interpreter lock: upper_out = seq upper-cased (ASCII),
 * fwd_out / rev_out = upper_out with 'M' at every called letter of every occurrence (overlapping ones included) of the
 * spec's motifs / of their reverse complements; all buffers n bytes. */
int mc_mark_iupac(const char *seq, int64_t n, const mc_iupac_spec *spec, char *upper_out, char *fwd_out, char *rev_out);

/* ===== pinned host memory, recycled =====
 * The DMA engines read a table at PCIe speed, beside running kernels, only from pinned memory.  Blocks handed back with
 * mc_host_free are kept (up to keep_bytes of idle memory) and handed out again: pinning costs page-table work per page, a
 * stream of shards allocates during its first two or three shards only.  With parser_uses_pool != 0 the columns of every
 * table parsed from then on (mc_parse_eventalign*) live in such blocks.  Without a GPU the blocks are plain memory. */
void *mc_host_alloc(int64_t bytes);
void mc_host_free(void *p);
int mc_host_is_pinned(const void *p);
int mc_host_pool_config(int32_t parser_uses_pool, int64_t keep_bytes);   /* keep_bytes < 0: unchanged (default 8 GiB) */

/* ===== native eventalign parser (host), replaces the line.split() ingest extract_contexts.py:140-152 ===== */
typedef struct mc_parsed mc_parsed;
/* Parses the byte range the reference's loop would consume for (startline, endline):
 * seek(max(startline-500,0)), readlines(8000000) batches while linepos <= endline-500 (:141-146).
 * Rows with < 12 tokens are dropped (:149-152); rows whose contig is not in contig_names are dropped
 * and recorded (the "could not find sequence" path :156-160).  The range is cut at line starts into one piece per
 * thread (n_threads > 0: exactly that many pieces; <= 0: one per core, pieces of at least 4 MB) and stitched in file order. */
int mc_parse_eventalign(const char *path, int64_t startline, int64_t endline,
                        const char *const *contig_names, int32_t n_contigs, int32_t n_threads,
                        mc_parsed **out);
/* The same for an exact byte range [byte_begin, byte_end) that starts at a line start (a piece of a file cut for several
 * GPUs), and the cutter: n_parts+1 offsets, every cut at the first line of a read (column 4 changes), pieces of similar
 * size -- a window never spans two reads (:179,:242), so pieces are scanned independently. */
int mc_parse_eventalign_range(const char *path, int64_t byte_begin, int64_t byte_end,
                              const char *const *contig_names, int32_t n_contigs, int32_t n_threads, mc_parsed **out);
int mc_eventalign_read_cuts(const char *path, int32_t n_parts, int64_t *cuts);
/* ... the same inside the byte range [lo, hi) (lo at a line start): cuts[0] = lo, cuts[n_parts] = min(hi, file size); and
 * the byte range the reference's batch loop consumes for (startline, endline) -- what mc_parse_eventalign parses (:141-148:
 * the last < 500 bytes of a file can stay unread) -- for callers that cut that range into shards. */
int mc_eventalign_read_cuts_range(const char *path, int64_t lo, int64_t hi, int32_t n_parts, int64_t *cuts);
/* ... at offsets of the caller's choosing (ascending, inside [lo, hi)): cuts[0] = lo, cuts[i + 1] = the first line of a read at or
 * behind want[i], cuts[n_want + 1] = min(hi, file size) -- a stream whose first shards are small (its pipeline fills sooner). */
int mc_eventalign_read_cuts_at(const char *path, int64_t lo, int64_t hi, const int64_t *want, int32_t n_want, int64_t *cuts);
int mc_eventalign_consumed_range(const char *path, int64_t startline, int64_t endline, int64_t *lo, int64_t *hi);
int mc_parsed_view(const mc_parsed *p, mc_table_view *out);
const char *mc_parsed_read_name(const mc_parsed *p, int32_t read_id);
int64_t mc_parsed_n_unknown(const mc_parsed *p);                 /* rows dropped for an unknown contig */
const char *mc_parsed_unknown_name(const mc_parsed *p, int64_t i); /* contig text of the i-th such row */
int32_t mc_parsed_n_pieces(const mc_parsed *p);                  /* pieces the range was cut into, one thread each */
void mc_parsed_free(mc_parsed *p);

/* ===== FASTQ read quality (replaces read_qual.py:6-19) =====
 * One (key, mean phred) pair per record, in file order: key = id.split(':')[0].split('_')[0] (:11-12), mean = exact
 * integer sum of (ASCII - 33) / count in float64 (np.mean of the phred list, :11).  A path containing ".gz" is inflated
 * (:7).  n_threads <= 0: one piece per core (pieces of at least 4 MB).  Errors (a title not starting with '@', a third
 * line not starting with '+', sequence and quality of different lengths) are the ValueErrors Biopython raises there. */
typedef struct mc_fastq mc_fastq;
int mc_fastq_read_quality(const char *path, int32_t n_threads, mc_fastq **out);
/* -> number of records; key_pool holds the keys, each followed by '\n'; key_off has n+1 offsets into it. */
int64_t mc_fastq_view(const mc_fastq *f, const char **key_pool, const int64_t **key_off, const double **mean);
void mc_fastq_free(mc_fastq *f);

/* ===== device context ===== */
typedef struct mc_ctx mc_ctx;
int mc_ctx_create(int device, mc_ctx **out);
/* One process per GPU on a multi-socket host: binds the calling thread (and the threads it starts later) to the cores of the
 * NUMA node the GPU is attached to, so that the pinned buffers of its contexts are allocated there.  Call before
 * mc_ctx_create.  -> node, or -1 if the topology is unknown (nothing changed).  Not an error code. */
int mc_bind_to_device_numa_node(int device);
void mc_ctx_destroy(mc_ctx *ctx);
int mc_ctx_set_reference(mc_ctx *ctx, const mc_ref_view *host_ref);          /* H2D, replaces :154-160 */
/* The same from the raw bases, the site masks made on the GPU (the FASTA site-LUT builder, extract_contexts.py:33-41,:60-81,
 * for a motif): host_ref->seq holds the FASTA bytes of EVERY contig (any case; ASCII), mbits_* are not read; motif_fwd /
 * repl_fwd: the motif and what str.replace puts in its place ('M' for the base), *_rev: for the reverse complement and the
 * complement base; 1..16 bases; the motifs must not be able to overlap themselves (no proper prefix is also a suffix -- then
 * "left to right, non-overlapping" is "every occurrence").  Leaves the device reference exactly as mc_ctx_set_reference
 * would with every contig marked (mc_ctx_fetch_reference copies it back: the parity tests). */
int mc_ctx_set_reference_motif(mc_ctx *ctx, const mc_ref_view *host_ref, const char *motif_fwd, const char *repl_fwd, int32_t m_fwd,
                               const char *motif_rev, const char *repl_rev, int32_t m_rev);
/* The same for a set of degenerate motifs (csrc/mc_iupac.h: every occurrence counts, a literal 'M' of the sequence stays a
 * mark on both strands): host_ref as above, with ceil(contig_len / 32) + 2 mask words per contig and the contigs' bases inside
 * seq[0, n_seq_bytes); spec: mc_iupac_spec_add.  Leaves the device reference exactly as mc_ctx_set_reference would with
 * every contig marked by mc_mark_iupac. */
int mc_ctx_set_reference_iupac(mc_ctx *ctx, const mc_ref_view *host_ref, const mc_iupac_spec *spec);
int mc_ctx_fetch_reference(mc_ctx *ctx, uint8_t *seq, int64_t n_seq_bytes, uint32_t *mbits_fwd, uint32_t *mbits_rev,
                           int32_t *rank_fwd, int32_t *rank_rev, int64_t n_words, int64_t *site_base, int64_t *n_sites);
int mc_ctx_upload_table(mc_ctx *ctx, const mc_table_view *host_table);        /* H2D of the columns; returns when done */
int mc_ctx_set_read_quality(mc_ctx *ctx, const double *qual, int32_t n_reads);/* read2qual, :163-166   */

/* ---- streaming distinct tables: a file as a sequence of shards (the reference's batch loop, :140-148) ----
 * A ctx holds MC_TABLE_SLOTS resident tables.  mc_ctx_upload_table_async ENQUEUES the upload of a table into a free slot
 * and makes it the current table (the one the passes enqueued afterwards scan): the columns travel on an upload stream of
 * their own (DMA, beside the kernels of earlier passes; the source should be pinned: mc_host_alloc / a parser table with
 * mc_host_pool_config(1, ..)); no kernel runs at upload -- the FIRST pass over a table validates it while it scans (are the
 * positions of every read non-decreasing, its event indices strictly monotone: what lets the window rule stand in for the
 * reference's sequential machine, :161-176), later passes over the same table use what it found.  read_qual
 * ([n_reads], read ids of THIS table; may be NULL: mc_ctx_set_read_quality applies) travels with the table.  No
 * hipMalloc / hipFree happens per table once the slots are big enough: mc_ctx_reserve_tables sizes them (and the per-pass
 * scratch and record sets) once for tables of up to max_rows rows, max_segs segments, max_reads reads; without it the
 * first table that needs more re-allocates (synchronising).  The host buffers must stay untouched until
 * mc_ctx_wait_upload(slot) returns.  (A table can also arrive as TEXT and be parsed on the device: mc_ctx_parse_begin below.)
 * A slot is free again when every pass that scanned its table has been handed out by
 * mc_wait_records (and the next pass after it: the last records handed out may still be reduced by mc_site_counts); with
 * no free slot the call fails with MC_E_NO_FREE_SLOT: wait for a pass first. */
#define MC_TABLE_SLOTS 12
int mc_ctx_reserve_tables(mc_ctx *ctx, int64_t max_rows, int32_t max_segs, int32_t max_reads);
int mc_ctx_upload_table_async(mc_ctx *ctx, const mc_table_view *host_table, const double *read_qual, int32_t *slot);
int mc_ctx_wait_upload(mc_ctx *ctx, int32_t slot);
int mc_ctx_current_slot(mc_ctx *ctx);                       /* slot of the current table, -1: none */
/* Makes the table resident in `slot` the current one again.  as_new != 0: the next pass treats it like a table it has never
 * seen -- it does everything the first pass over a table does (positions and event indices streamed, every row validated),
 * whatever earlier passes learned (measurement: the cost of a table that is scanned once, without the upload).  Fails for a
 * slot that holds no COMPLETE table (never filled; a parse abandoned or never finished).  Passes over the slot that are in
 * flight keep the plan they were enqueued with: declare a table new beside them only if they are first passes too. */
int mc_ctx_select_table(mc_ctx *ctx, int32_t slot, int32_t as_new);
/* hipEvent time of the last upload into `slot` (waits for it): the H2D transfers, in ms.  *validate_ms is 0: nothing runs at
 * upload any more (the validation is part of the first pass's scan). */
int mc_ctx_upload_times_ms(mc_ctx *ctx, int32_t slot, float *h2d_ms, float *validate_ms);
/* hipEvent times of the last mc_ctx_parse_begin into `slot` (waits for it; call between mc_ctx_parse_begin and
 * mc_ctx_parse_finish / _abandon): *text_h2d_ms the transfer of the shard's text, *parse_ms the device parser's kernels behind
 * it (kp_count .. kp_place and the small copies that hand the result out) -- what replaces the reference's `line.split()` loop
 * (extract_contexts.py:146-152).  Meaningful when nothing else was in flight on the parse stream (bench.py's roofline_parser). */
int mc_ctx_parse_times_ms(mc_ctx *ctx, int32_t slot, float *text_h2d_ms, float *parse_ms);
/* MLP weights, row-major float64: W1[n_in*n_hidden], b1[n_hidden], W2[n_hidden], b2[1] per sub-model (at most 8 sub-models:
 * the reference's models have two, 'MG' and 'MH', or one); submodel_of_char[256]: context[k] (ASCII) -> sub-model index,
 * 255 = KeyError path (:197,:218). */
int mc_ctx_set_mlp(mc_ctx *ctx, int32_t n_models, int32_t n_in, int32_t n_hidden,
                   const double *W1, const double *b1, const double *W2, const double *b2,
                   const uint8_t *submodel_of_char);

/* Random forest (classifier RF, train_model.py:39-45; same call site :199): trees flattened, node arrays concatenated.
 * model_tree_off[n_models+1]: first tree of each sub-model; tree_node_off[n_trees+1]: root of each tree; left/right: child
 * node (absolute index) or -1 at a leaf; value[2*node .. 2*node+1]: the node's two class values.  Inputs are cast to
 * float32 before the comparisons `x[feature] <= threshold`, as scikit-learn does; p = mean over trees of v1/(v0+v1). */
int mc_ctx_set_forest(mc_ctx *ctx, int32_t n_models, int32_t n_in, const int32_t *model_tree_off,
                      const int32_t *tree_node_off, const int32_t *left, const int32_t *right, const int32_t *feature,
                      const double *threshold, const double *value, const uint8_t *submodel_of_char);

/* The closed-form classifiers of `-c LR` / `-c NBC` (train_model.py:55-60: LogisticRegression, GaussianNB; scored at the same
 * call site, :199).  params: n_models * stride doubles --
 *   MC_CLF_LOGISTIC, stride n_in + 1:   coef_[0][0..n_in), intercept_[0]              p = expit(x . coef + intercept)
 *   MC_CLF_GNB,      stride 4 n_in + 2: theta_[0], var_[0], theta_[1], var_[1] (n_in each), log(class_prior_[0]), log(class_prior_[1])
 *                                       p = exp(jll_1 - logsumexp(jll)), jll_c = log prior_c - 0.5 sum log(2 pi var_c) - 0.5 sum (x - theta_c)^2 / var_c
 * fp64, sums in index order.  Replaces the MLP / forest of the context. */
#define MC_CLF_LOGISTIC 1
#define MC_CLF_GNB 2
int mc_ctx_set_simple_classifier(mc_ctx *ctx, int32_t kind, int32_t n_models, int32_t n_in, const double *params, int32_t stride,
                                 const uint8_t *submodel_of_char);

/* RBF support-vector classifier of `-c SVM` (train_model.py:51-53: SVC(kernel='rbf', probability=True), two classes, dense; same call
 * site :199), scored as scikit-learn's libsvm does.  Sub-models have different numbers of support vectors: model_sv_off[n_models+1]
 * gives each sub-model's first one (model_sv_off[0] = 0); sv[n_sv_total*n_in]: the support vectors, row by row;
 * dual_coef[n_sv_total]: their coefficients as scikit-learn hands them to libsvm (`_dual_coef_[0]`); params[n_models*4]: per
 * sub-model gamma (resolved, `_gamma`), intercept (`_intercept_[0]`), A, B (`_probA[0]`, `_probB[0]`).
 *   dec = sum_i dual_coef_i exp(-gamma sum_j (x_j - sv_ij)^2) + intercept   (support-vector order)
 *   s   = Platt sigmoid of dec * A + B, clamped to [1e-7, 1 - 1e-7]
 *   p   = libsvm's iterative pairwise coupling for two classes (r01 = s), the probability of classes_[1]
 * fp64.  At most 8 sub-models.  Replaces the MLP / forest / closed-form classifier of the context. */
int mc_ctx_set_svm(mc_ctx *ctx, int32_t n_models, int32_t n_in, const int32_t *model_sv_off, const double *sv,
                   const double *dual_coef, const double *params, const uint8_t *submodel_of_char);

typedef struct mc_params {
    int32_t k;             /* -n   (:110 `k`)            */
    int32_t skip_thresh;   /* -s   (:183,242)            */
    double  qual_thresh;   /* -q   (:167)                */
    int32_t tail_contig;   /* contig id of the first unfiltered row AFTER this table (next shard), or -1
                              if none: the last window is then lost, as at EOF (R6)                  */
    int32_t score;         /* 1: run the classifier (predict mode); 0: features only (--train)     */
    int32_t entry_read;    /* read id `last_read` holds when the table starts (-1: none), and      */
    int32_t entry_first_idx; /* the matching first_read_ind (:161-162); shards > 0 of one file      */
} mc_params;

/* How the pass handed out last by mc_wait_records ran: *fused_room > 0 -- scan, ordering and emit as ONE kernel with that many
 * record slots per 960-row piece (dense references: k1_fused; the slots a piece does not fill never reach the host);
 * *rerun != 0 -- the pipelined pass could not be finished as enqueued (record room too small, an irregular read, a row that
 * contradicts what a block was classified on) and was repeated synchronously inside mc_wait_records. */
int mc_last_pass_info(mc_ctx *ctx, int32_t *fused_room, int32_t *rerun);
/* What the scan of the pass enqueued last streams (tests): 0 positions, index relations and model-N bits, every row validated;
 * 1 positions and model-N bits; 2 unit summaries; 3 unit summaries and both relation columns, every row validated; -1 no pass
 * yet.  A pass that was repeated synchronously inside mc_wait_records leaves the repeat's mode. */
int mc_ctx_last_scan_mode(mc_ctx *ctx);
/* Which tiles of the current table the scan takes in a single batch when it streams unit summaries (modes 2 and 3; tests): the
 * name-block descriptors of the SYNCHRONOUS pass run last over this table (mc_extract_features) and the tiles' first blocks are
 * copied to the host and the scan's own predicate (scan_tile_is_whole, mc_dev.h) is evaluated per tile of 2048 rows.  Returns the
 * number of tiles for which it holds, negative on error; per_tile (NULL, or a byte per tile): 1 where it holds, else 0.  (A tile
 * for which it holds but which lists more than 64 units is taken by the general loop all the same.) */
int64_t mc_ctx_whole_tiles(mc_ctx *ctx, uint8_t *per_tile);
/* The rows of a pipelined pass as TEXT, made on the device (mc_rowtext.hip; replaces mc_format_diffs on the host, the row writer of
 * extract_contexts.py:207-216).  mc_ctx_row_text(on = 1, the two labels of :200-206; on = 2 at the start of a stream: also takes back the
 * blocks an earlier stream never released -- nobody may be reading them any more): the passes enqueued from now on also print their
 * records where they are -- the packed records, the read names in the shard's text (tables the device parser made:
 * mc_ctx_parse_begin .. _finish), the contig names, the marked reference, shortest round-trip digits in integer arithmetic
 * (mc_rowtext.h) -- and send the text to pinned host memory behind the records.  After mc_wait_records, mc_last_row_text says
 * where: *text / *n_bytes / *n_rows, and *block >= 0 -- a handle (the block and the ticket it was taken with: one that is given back twice, or
 * after a later stream began, frees nothing) --, which the caller gives back with mc_row_text_release (any thread) once it
 * has written the rows; *block < 0: this pass has none (not asked for, another kind of table, no free block, or a record the
 * device does not print -- a context that leaves the contig, an unknown sub-model key, an unscored record, a number outside
 * [1e-29, 1e9): the reference's exit paths and the host formatter's general cases) and mc_format_diffs makes the rows as before. */
int mc_ctx_row_text(mc_ctx *ctx, int32_t on, const char *label_meth, const char *label_unmeth);
int mc_last_row_text(mc_ctx *ctx, const char **text, int64_t *n_bytes, int64_t *n_rows, int32_t *block);
int mc_row_text_release(mc_ctx *ctx, int32_t block);
/* The row writer's number printing alone, on the device (tests).  The doubles v[0, n) go through the row writer's digit kernel, the first
 * n / 2 as wide slot means, the rest as read qualities; then fixed[0, n_fixed) as integer slot means (repr(d / 1e4)) and prob[0, n_prob)
 * as np.round(p, 2), through the same sinks the rows use.  Item i (numbers, then fixed, then prob) is written at text[i * 48 + (i + shift)
 * % 8] (every start alignment; text: 48 bytes an item, filled with 0xA5 first); len[i] = the length the counting pass gives it, ok[i] =
 * 1 if it is printed (0: the row would go to the host formatter -- nothing written, len -1).  shift >= 0. */
#define MC_ROWTEXT_PROBE_STRIDE 48
int mc_ctx_rowtext_probe(mc_ctx *ctx, const double *v, int64_t n, const int32_t *fixed, int64_t n_fixed, const double *prob, int64_t n_prob,
                         int32_t shift, char *text, int32_t *len, uint8_t *ok);
/* The hot path on the GPU: strand resolve + window scan + classifier.  Leaves the flush records on the
 * device, in file order; *n_records = how many. */
int mc_extract_features(mc_ctx *ctx, const mc_params *prm, int64_t *n_records);
/* The records of the last mc_extract_features, copied into caller buffers (capacity >= n_records) ... */
int mc_fetch_records(mc_ctx *ctx, const mc_calls_view *host_out);
/* ... or as a view of the context's own pinned host buffers (no copy; valid until the next call on this ctx;
 * capacity is set to the record count).  mc_extract_features already moved them there, overlapped with the classifier. */
int mc_fetch_records_view(mc_ctx *ctx, mc_calls_view *out);
/* Pipelined passes, for callers that stream many tables / shards (or the same table, as bench.py does): a pass is only
 * ENQUEUED -- strand resolve, scan + emit, classifier, packing of what is copied out, all on the ctx stream, each
 * pass with its own counters, strand-resolve output and record set -- and copied out (one DMA transfer: the narrow columns
 * of the n records, then slot means and probabilities of the records that are calls, see mc_calls_view.call_row) when it
 * is waited for, beside the kernels of the passes behind it; no host round trip sits inside a pass.  At
 * most six passes are in flight (one being copied out, one in the side stream's kernels, one computing, the others queued).  mc_wait_records hands out the
 * OLDEST pass and returns a view of the context's pinned buffers (valid until six more passes have been enqueued).  A
 * pass that needs more than the fast path (irregular reads, record buffers too small) is re-run synchronously inside
 * mc_wait_records -- results are the same, only slower.  Either classifier (MLP: k2_mlp, forest: k3_forest) runs on the side
 * stream behind the pass's emit. */
int mc_extract_features_async(mc_ctx *ctx, const mc_params *prm);
int mc_wait_records(mc_ctx *ctx, int64_t *n_records, mc_calls_view *out);
/* Optional first half of mc_wait_records, for the oldest pass in flight whose copy-out has not been started: waits for
 * its kernels, reads its counters and ENQUEUES its copy-out without waiting for it.  Calling it for pass i+1 before
 * mc_wait_records(pass i) keeps the DMA engine busy back to back (bench.py does).  No-op if every pass is being copied. */
int mc_wait_records_begin(mc_ctx *ctx);
/* Kernel times of the last mc_extract_features, from hipEvents on the ctx stream, in ms:
 * [0] strand resolve (K0), [1] window scan (k1_scan), [2] window emit (k1_group_scan + k1_list + k1_emit),
 * [3] classifier (K2), [4] total. */
int mc_last_times_ms(mc_ctx *ctx, float *out5);
/* Pipelined passes: the two hipEvents that only TIME a pass (start of K0, start of the scan) are recorded with every n-th
 * pass (default 1 = every pass, 0 = never).  An event between two kernels costs the queue about 9 us on this GPU, 6 % of a
 * pass of the headline workload.  mc_last_pass_timed: 1 if the pass mc_wait_records handed out last carried them, i.e.
 * mc_last_times_ms is about that pass; for an untimed pass mc_last_times_ms keeps the values of the last timed one. */
int mc_ctx_set_pass_timing(mc_ctx *ctx, int every_n);
int mc_last_pass_timed(mc_ctx *ctx);
int mc_ctx_sync(mc_ctx *ctx);

/* Batched classifier alone (B2, extract_contexts.py:199): X[n*n_in] -> p[n]; host buffers. */
int mc_mlp_forward(mc_ctx *ctx, const double *X, const uint8_t *submodel, int64_t n, double *p);
int mc_forest_forward(mc_ctx *ctx, const double *X, const uint8_t *submodel, int64_t n, double *p);
int mc_simple_forward(mc_ctx *ctx, const double *X, const uint8_t *submodel, int64_t n, double *p);     /* LR / NBC */
int mc_svm_forward(mc_ctx *ctx, const double *X, const uint8_t *submodel, int64_t n, double *p);        /* SVM */

/* ===== per-site reduction feeding make_bed (make_bed.py:86-96,:134,:143,:154), the one exchange step of a multi-GPU job =====
 * Sites = every 'M' of the marked strands, numbered per contig: '+' sites by position, then '-' sites by position
 * (mcaller_amd.make_bed.SiteIndex uses the same order).  Each rank reduces the records of its own last
 * mc_extract_features call on the device; mc_site_allreduce sums the counts and takes the minimum first-seen row over
 * the ranks with ncclAllReduce (RCCL over xGMI; librccl.so is loaded on first use) and copies the result out. */
#define MC_UNIQUE_ID_BYTES 128
int64_t mc_site_count(mc_ctx *ctx);                       /* number of marked sites of the reference in the ctx */
/* counts of this rank: n_meth / n_total per site (label 'm..' <=> p >= 0.5, :200) and the smallest close_row +
 * row_offset (global row of the first occurrence, :134).  Two kinds of records are left out and counted for the caller:
 * *n_pending -- probability NaN on the device (the host scored them): add them with mc_site_counts_add;
 * *n_cross_contig -- closed by a row of ANOTHER contig than the site's (tail_contig: the contig of the row after this
 * table, as in mc_params): make_bed keys such a row on the closing row's contig (R8, :216), which is no site of the
 * numbering -- the caller adds them to the BED as rows of their own. */
int mc_site_counts(mc_ctx *ctx, int64_t row_offset, int32_t tail_contig, int64_t *n_pending, int64_t *n_cross_contig);
/* The same over the passes of a streamed file: mc_site_counts_reset zeroes the counts, mc_site_counts_accumulate adds the
 * records of the pass handed out last (mc_wait_records) -- row_offset: the rows of the shards before it, so that the first-seen
 * rows stay in file order.  mc_site_counts == reset + accumulate. */
int mc_site_counts_reset(mc_ctx *ctx);
int mc_site_counts_accumulate(mc_ctx *ctx, int64_t row_offset, int32_t tail_contig, int64_t *n_pending, int64_t *n_cross_contig);
int mc_site_counts_add(mc_ctx *ctx, const int64_t *site, const uint8_t *is_meth, const int64_t *first_row, int64_t n);
int mc_comm_available(void);                              /* 0: librccl.so can be loaded in this process (nothing else is touched) */
int mc_comm_unique_id(uint8_t *out128);                   /* rank 0: ncclGetUniqueId; ship the bytes to every rank */
int mc_comm_init(mc_ctx *ctx, int32_t world, int32_t rank, const uint8_t *unique_id128);   /* ncclCommInitRank */
int mc_comm_destroy(mc_ctx *ctx);
/* all-reduce (if a communicator with world > 1 is set) + D2H: n_meth[n], n_total[n] int32, first_row[n] int64
 * (INT64_MAX: site not seen); *ms = time of the two collectives (hipEvents). */
int mc_site_allreduce(mc_ctx *ctx, int32_t *n_meth, int32_t *n_total, int64_t *first_row, float *ms);
/* This rank's own counts as they stand (D2H only, no collective): what a job adds up on the host when a rank could not
 * take part in the all-reduce. */
int mc_site_counts_fetch(mc_ctx *ctx, int32_t *n_meth, int32_t *n_total, int64_t *first_row);

/* ===== the classifier fit behind --train (train_model.py:47,:62-65,:81-100): one-hidden-layer tanh/logistic perceptron, =====
 * Adam, binary log-loss + L2, scikit-learn's MLPClassifier recipe (batches of min(200, n) rows, tol / n_iter_no_change
 * stopping).  n_jobs independent fits run side by side, one workgroup each (the 5 GroupKFold fits + the final fit of a
 * sub-model); job j trains on rows train_idx[train_off[j] .. train_off[j+1]) of X and is scored (accuracy, p > 0.5) on
 * rows val_idx[val_off[j] .. val_off[j+1]).  Start weights: `init` ([n_jobs][n_in*n_hidden + 2*n_hidden + 1]: W1
 * row-major, b1, W2, b2) or, if NULL, Glorot-uniform from seeds[j] (NULL: seed + j).  The epoch order is a keyed
 * permutation of the row index (shuffle != 0) or the given order. */
typedef struct mc_fit_params {
    int32_t n_in, n_hidden;        /* k+1 inputs (<= MC_MAX_K+1), hidden units (<= 128; reference: 100)  */
    int32_t batch_size;            /* scikit-learn 'auto': min(200, n); the kernel clamps to each job's n */
    int32_t max_iter;              /* 200 */
    int32_t n_iter_no_change;      /* 10  */
    int32_t shuffle;               /* 1   */
    double alpha, lr_init, beta1, beta2, epsilon, tol;   /* 0.001 (train_model.py:47), 0.001, 0.9, 0.999, 1e-8, 1e-4 */
    uint64_t seed;
} mc_fit_params;
int mc_mlp_fit(mc_ctx *ctx, const mc_fit_params *prm, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_jobs,
               const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx,
               const uint64_t *seeds, const double *init,
               double *W1, double *b1, double *W2, double *b2,      /* per job: [n_in*n_hidden], [n_hidden], [n_hidden], [1] */
               double *loss_curve /* [n_jobs*max_iter] */, int32_t *n_iter /* epochs run */, int64_t *val_correct);

/* ===== the random-forest fit behind --train -c RF (train_model.py:39-45,:62-65,:92-100): scikit-learn's RandomForestClassifier =====
 * (entropy, bootstrap) with keyed randomness (tests/forest_fit_oracle.py defines it; the kernel follows it bit for bit).  n_jobs x
 * n_trees independent trees, a workgroup each (k5_forest_fit).  Job j fits on rows train_idx[train_off[j] .. train_off[j+1]) of X
 * (n_samples x n_in, cast to float32), labels y in {0, 1}, seed seeds[j]; its trees score rows val_idx[val_off[j] .. val_off[j+1])
 * (val_correct[j]: predictions p1 > p0 equal to y).  G[n_G]: G[m] = m ln m, G[0] = 0, n_G > the largest job's row count.
 * Output: the trees one after the other (tree j*n_trees + t), nodes in depth-first pre-order with scikit-learn's fields and child
 * links local to the tree (-1 at a leaf; feature -2, threshold -2.0 there); tree_node_off[n_jobs*n_trees+1]; value[2*node+c]: the
 * weighted class fractions.  node_cap: room in the node arrays, at least the sum over jobs of n_trees * min(2^(max_depth+1) - 1,
 * 2 * rows - 1).  Returns -12 on a parameter out of range (max_features > n_in included). */
typedef struct mc_forest_params {
    int32_t n_in;                  /* features, 1 .. MC_MAX_K+1                    */
    int32_t n_trees;               /* 50   (1 .. 100000)                           */
    int32_t max_depth;             /* 10   (1 .. 30: heap ids stay in 64 bits)     */
    int32_t max_features;          /* 4    (1 .. n_in)                             */
    int32_t min_samples_split;     /* 3    (>= 2)                                  */
    int32_t min_samples_leaf;      /* 2    (>= 1)                                  */
    int32_t bootstrap;             /* 1    (0: every training row once)            */
} mc_forest_params;
int mc_forest_fit(mc_ctx *ctx, const mc_forest_params *prm, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_jobs,
                  const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx,
                  const uint64_t *seeds, const double *G, int64_t n_G, int64_t node_cap, int64_t *tree_node_off,
                  int32_t *left, int32_t *right, int32_t *feature, double *threshold, double *value, double *impurity,
                  int32_t *n_node_samples, double *weighted_n_node_samples, int64_t *val_correct);
/* How the last mc_forest_fit call on the context that reached the device ran.  The trees are grown `batch` at a time, as many as
 * fit MCALLER_FOREST_MEM_MB (default 4096; read once per process) of per-tree work arrays: batch = max(1, min(n_trees_total,
 * MB * 2^20 / per_tree_bytes)), n_batches launches of k5_forest_fit, the last one with the remainder.  All zero before the first
 * call; a call refused with -12 leaves the figures of the call before. */
typedef struct mc_forest_fit_stats {
    int64_t n_batches;             /* launches of k5_forest_fit                              */
    int64_t batch;                 /* trees (workgroups) of a full batch                     */
    int64_t per_tree_bytes;        /* work memory of one tree                                */
    int64_t n_trees_total;         /* n_jobs * n_trees                                       */
    int64_t n_nodes;               /* nodes written over all trees (0 if the call failed)    */
} mc_forest_fit_stats;
int mc_forest_fit_last_stats(mc_ctx *ctx, mc_forest_fit_stats *out);

/* ===== the RBF support-vector fit behind --train -c SVM (train_model.py:51-53,:62-65,:92-101): scikit-learn's SVC(kernel='rbf') =====
 * solved as libsvm's Solver does without shrinking (tests/svm_fit_oracle.py restates it): n_jobs independent solves, a workgroup each
 * (k6_svm_fit).  Job j solves on rows train_idx[train_off[j] .. train_off[j+1]) of X (n_samples x n_in, fp64), labels y in {0, 1},
 * RBF width gamma[j]; the rows arrive in the order libsvm solves them, grouped by the sub-problem's sorted labels: the class of the
 * job's first row is the solve's +1.  Output per training entry alpha >= 0 (the dual coefficient is +alpha on +1 rows, -alpha on -1
 * rows), per job rho (the intercept is -rho), n_iter and status (0: converged, 1: stopped at the iteration cap).  The job's held-out
 * rows val_idx[val_off[j] .. val_off[j+1]) get val_dec, k3_svm's decision value turned so that > 0 means class 0 (libsvm's
 * dec * label[0]), and val_correct[j] counts the rows whose prediction (class 0 iff val_dec > 0) equals y.  Returns -12 on a parameter
 * out of range: n_in outside 1..64, C or tol <= 0, a job with fewer than two rows or one class, more than 2^26 rows, or more than
 * 4 GiB of device work memory. */
typedef struct mc_svm_params {
    double C;                      /* 1.0   (> 0)                                          */
    double tol;                    /* 1e-3  (> 0): stop when Gmax + Gmax2 < tol             */
    int64_t max_iter;              /* 0: max(10^7, 100 * rows) per job                     */
} mc_svm_params;
int mc_svm_fit(mc_ctx *ctx, const mc_svm_params *prm, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in, int32_t n_jobs,
               const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx, const double *gamma,
               double *alpha, double *rho, int64_t *n_iter, int32_t *status, int64_t *val_correct, double *val_dec);
/* libsvm's sigmoid_train (the Platt parameters A, B of svm_binary_svc_probability) on the device, one workgroup with fixed-order sums:
 * dec[n] decision values, y[n] = 0 for label +1 (libsvm's prior1: classes_[0]), 1 for -1. */
int mc_svm_sigmoid_train(mc_ctx *ctx, const double *dec, const uint8_t *y, int64_t n, double *A, double *B);

/* ===== the logistic-regression fit behind --train -c LR (train_model.py:55-57,:62-65,:92-101): scikit-learn's ======================
 * LogisticRegression(solver='liblinear', penalty='l1') -- liblinear's solve_l1r_lr (newGLMNET; tests/lr_fit_oracle.py restates it):
 * n_jobs independent fits, a workgroup each (k7_lr_fit).  Job j fits on rows train_idx[train_off[j] .. train_off[j+1]) of X
 * (n_samples x n_in, fp64, finite), labels y in {0, 1}; the rows may come in any order (the fit takes classes_[0]'s first, stable,
 * as liblinear's group_classes does) and must hold both classes.  The bias is a column of 1.0 penalised like the other weights
 * (intercept_scaling = 1).  seeds[j]: the 31-bit seed of the fit's std::mt19937 (the QP shuffle), scikit-learn's
 * RandomState.randint(2^31 - 1).  Output per job: coef[j*n_in .. +n_in) (toward class 1), intercept[j], n_iter[j] (Newton
 * iterations) and status[j] (1: max_iter was reached, scikit-learn's ConvergenceWarning).  The held-out rows
 * val_idx[val_off[j] .. val_off[j+1]) get val_dec (k3_simple's decision value: the dot product in index order, plus the
 * intercept), and val_correct[j] counts those whose prediction (class 1 iff val_dec > 0) equals y.  Returns -12 on a parameter out
 * of range: n_in outside 1..64, C or tol not finite and > 0, max_iter outside 1..10^6, a job with fewer than two rows or one
 * class, an index outside the rows, more than 2^26 rows, or more than 4 GiB of device work memory. */
typedef struct mc_lr_params {
    double C;                      /* 1.0   (> 0)                                          */
    double tol;                    /* 1e-4  (> 0): liblinear's eps before its pos/neg scaling */
    int32_t max_iter;              /* 100   Newton iterations                              */
    int32_t pad;
} mc_lr_params;
int mc_lr_fit(mc_ctx *ctx, const mc_lr_params *prm, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in, int32_t n_jobs,
              const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx, const uint32_t *seeds,
              double *coef, double *intercept, int32_t *n_iter, int32_t *status, int64_t *val_correct, double *val_dec);

/* ===== the Gaussian naive Bayes fit behind --train -c NBC (train_model.py:59-60,:62-65,:92-101): scikit-learn's GaussianNB() =====
 * n_jobs independent fits, a workgroup each (k7_nb_fit), on the same job layout as mc_lr_fit (both classes in every job).  Output per
 * job: theta[j*2*n_in ..] and var[j*2*n_in ..] ([class][feature]: the means and the centred variances plus epsilon_, as GaussianNB
 * stores var_), epsilon[j] = var_smoothing * the largest per-feature variance of the job's rows, class_count[2*j + c]; the held-out
 * rows are predicted as k3_simple scores them (argmax of the joint log-likelihood, ties to class 0) and val_correct[j] counts the
 * right ones.  Returns -12 on what mc_lr_fit refuses, on var_smoothing not finite and > 0, and on a job whose training rows are all
 * equal (epsilon_ = 0; the other outputs are written then). */
typedef struct mc_nb_params {
    double var_smoothing;          /* 1e-9  (> 0)                                          */
} mc_nb_params;
int mc_nb_fit(mc_ctx *ctx, const mc_nb_params *prm, const double *X, const uint8_t *y, int64_t n_samples, int32_t n_in, int32_t n_jobs,
              const int64_t *train_off, const int32_t *train_idx, const int64_t *val_off, const int32_t *val_idx, double *theta,
              double *var, double *epsilon, int64_t *class_count, int64_t *val_correct);

/* ===== the eventalign text parsed on the GPU (replaces the row ingest, extract_contexts.py:140-152, for streamed shards) =====
 * The host only moves bytes: mc_read_file_range preads a byte range into (pinned) memory with all cores;
 * mc_ctx_parse_begin sends it and enqueues the kernels that split it into lines, tokenise (str.split()'s ASCII whitespace,
 * first 12 tokens), convert (int(); floats in plain decimal form as units of 1e-4) and write the columns of a free table
 * slot; mc_ctx_parse_end waits and hands out what the host needs for names: segments (first row, contig id, where the read
 * name stands in the text, whether it starts a name block), the contig tokens the reference does not hold (file order) and
 * the flag column; mc_ctx_parse_finish takes read ids and qualities: the slot is now what mc_ctx_upload_table_async would
 * have left (current table).  status 1: the shard holds something this path does not reproduce bit for bit (a number form
 * that needs strtod, a value out of range, more rows or segments than the slot holds; mc_last_error says which) -- call
 * mc_ctx_parse_abandon and parse it with mc_parse_eventalign_range.  begin for the next shard may be called before end. */
typedef struct mc_devparse_result {
    int32_t status;
    int64_t n_lines, n_rows;
    int32_t n_seg, n_unknown;
    const int64_t *seg_row_begin;     /* [n_seg] ascending                                              */
    const int32_t *seg_contig;        /* [n_seg]                                                        */
    const int64_t *seg_name_off;      /* [n_seg] offset of the segment's read name in the text          */
    const int32_t *seg_name_len;
    const uint8_t *seg_name_start;    /* [n_seg] 1: first segment of a name block (MC_F_NAME_START)     */
    const int64_t *unknown_off;       /* [n_unknown] contig tokens of skipped lines (:156-160)          */
    const int32_t *unknown_len;
    const uint8_t *flags;             /* [n_rows] host copy of the flag column (pinned, owned by ctx)   */
} mc_devparse_result;
int mc_read_file_range(const char *path, int64_t byte_begin, int64_t byte_end, char *dst, int32_t n_threads);
/* ... or WITHOUT the copy: the range mapped from the page cache and registered for the DMA engines (a streamed shard's text goes
 * to the GPU from where the kernel keeps it).  *ptr points at byte `lo`; valid until mc_unmap_file_range(*handle).  Returns
 * non-zero where the runtime cannot register the mapping (no GPU ...): read the range with mc_read_file_range then. */
int mc_map_file_range(const char *path, int64_t lo, int64_t hi, void **handle, const char **ptr);
void mc_unmap_file_range(void *handle);
int mc_ctx_parse_begin(mc_ctx *ctx, const char *text, int64_t n_bytes, const char *const *contig_names, int32_t n_contigs,
                       int64_t max_rows, int32_t *slot);
int mc_ctx_parse_end(mc_ctx *ctx, int32_t slot, mc_devparse_result *out);
int mc_ctx_parse_finish(mc_ctx *ctx, int32_t slot, const int32_t *seg_read, int32_t n_reads, const double *read_qual);
int mc_ctx_parse_abandon(mc_ctx *ctx, int32_t slot);
/* The columns of the table in `slot` copied back to the host (any may be NULL) -- what the parity tests compare. */
int mc_ctx_fetch_columns(mc_ctx *ctx, int32_t slot, int64_t n_rows, int32_t *pos, int32_t *event_model_e4, int32_t *event_idx,
                         uint8_t *flags);
/* ... and its model-N bit column: ceil(n_rows / 8) bytes (bits at or beyond n_rows are whatever the slot holds there). */
int mc_ctx_fetch_model_n_bits(mc_ctx *ctx, int32_t slot, int64_t n_rows, uint8_t *out);
/* ... and its index-relation column: ceil(n_rows / 8) words (bits at or beyond n_rows are whatever the slot holds there). */
int mc_ctx_fetch_idx_rel_bits(mc_ctx *ctx, int32_t slot, int64_t n_rows, uint16_t *out);
/* ... its position-relation column, which the table's maker on the device writes with the positions: ceil(n_rows / 8) words,
 * row r = 8u + e: bit e of word u is pos[r] < pos[r-1] (the row before it in the table; row 0: clear), bit 8 + e is
 * pos[r] == 0 (bits at or beyond n_rows: 0). */
int mc_ctx_fetch_pos_rel_bits(mc_ctx *ctx, int32_t slot, int64_t n_rows, uint16_t *out);
/* ... and its unit summaries: ceil(n_rows / 8) pairs of int32, the positions of the first and the last row of every unit of
 * eight rows (the second of a last, partial unit is unspecified). */
int mc_ctx_fetch_unit_summaries(mc_ctx *ctx, int32_t slot, int64_t n_rows, int32_t *out);

/* ===== native `.diffs.<k>` row formatter (host), replaces the text assembly of the flush, extract_contexts.py:186-216 ===== */
typedef struct mc_format_args {
    const mc_calls_view *rec;          /* flush records in host memory (mc_fetch_records / _view)                  */
    int64_t n_records;
    int32_t k;
    const mc_table_view *table;        /* seg_row_begin / seg_read / seg_contig are read                           */
    const mc_ref_view *ref;            /* bases + strand masks: the marked strings the context is sliced from :194 */
    const char *const *contig_names;   /* [ref->n_contigs]                                                         */
    const char *const *read_names;     /* [table->n_reads] column 2 of the row                                :216 */
    const char *const *read_qual_txt;  /* [table->n_reads] str(read2qual[...]), the k+1-th feature        :189-193 */
    const char *tail_chrom;            /* chrom of records closed by the next shard's first row (or NULL)          */
    const char *label_meth;            /* 'm6A' / 'm'+base                                                :200-204 */
    const char *label_unmeth;          /* base                                                                :206 */
    const uint8_t *submodel_of_char;   /* [256] as in mc_ctx_set_mlp; 255 = the KeyError path             :218-223 */
} mc_format_args;
/* Rows of records [first, *stop_at) as one malloc'ed text block (release with mc_free); records flagged
 * MC_I_TOO_MANY produce no row.  *stop_at < n_records: that record needs the host's own handling (context leaving the
 * contig, NaN probability, unknown sub-model key or complement, centre not 'M': the reference's exit/crash paths). */
int mc_format_diffs(const mc_format_args *args, int64_t first, int32_t n_threads, char **text, int64_t *n_bytes,
                    int64_t *n_rows, int64_t *stop_at);
/* What records [0, n) add to the reference's counters, in one pass: counts3 = records with MC_I_TOO_MANY (:239), calls with an empty
 * slot (:234-238), records with MC_I_MULTI (:247-248) -- the SIZES of the reference's sets of (read, site) pairs if *ascending comes
 * back 1 (every pair new: a table whose read names do not repeat; seg_read[n_seg]: the read of every segment), otherwise the caller
 * counts distinct pairs itself -- and the positions of the calls (:235): pos_marks[p] = 1 for every call at site position p < n_marks,
 * *pos_min / *pos_top = smallest position / largest + 1 (a caller whose marks are too short grows them and calls again).  counts3 and
 * pos_marks may be NULL. */
int mc_count_records(const mc_calls_view *rec, int64_t n, const int32_t *seg_read, int64_t n_seg, int64_t *counts3, int32_t *ascending,
                     uint8_t *pos_marks, int64_t n_marks, int64_t *pos_min, int64_t *pos_top);
/* The columns mc_wait_records does not send, rebuilt on the host (all cores): call_row_out[n] (see mc_calls_view.call_row),
 * close_row_out[n] (64-bit closing rows), feats_out[n_call_rows * k] (the slot means as doubles); any may be NULL. */
int mc_calls_expand(const mc_calls_view *rec, int64_t n_records, int32_t k, int32_t *call_row_out, int64_t *close_row_out,
                    double *feats_out);
/* The four record columns in full from either layout of a view (narrow records: mc_calls_view.close_lo16; all cores):
 * site_pos_out[n], site_seg_out[n], info_out[n], close_row_out[n]; any may be NULL.  -12: a run list that does not begin at
 * record 0, does not ascend or leaves [0, n). */
int mc_records_expand(const mc_calls_view *rec, int64_t n_records, int32_t *site_pos_out, int32_t *site_seg_out, uint32_t *info_out,
                      int64_t *close_row_out);
void mc_free(void *p);
/* repr(float) == str(np.float64) of one value into out32 (NUL-terminated); returns its length. */
int mc_repr_double(double v, char *out32);
/* ... of d / 1e4 for a 32-bit integer d, from the integer alone (how the formatter prints the slot means that travel as
 * integers, mc_calls_view.feats_lo32): the same characters as mc_repr_double((double)d / 1e4). */
int mc_repr_fixed4(int32_t d, char *out32);
/* repr(v) by the device row writer's digit generation (mc_rowtext.h), built for the host: the same characters as mc_repr_double for
 * 1e-29 <= |v| < 1e9 and for zero; -> length, -1: a double it does not print. */
int mc_repr_double_rowtext(double v, char *out32);

/* ===== what the calls below that take whole text files through the GPU read from: a host text or a regular file =====
 * A file is read in pinned blocks (mc_read_file_range) while the block before is on its way to the device; its bytes give what
 * the same bytes as a text give.  Every source of a call is taken on its own: a file may stand beside a text.  A call returns
 * -12 for a source that is null where one is required, has a text and a path, n_bytes < 0, or n_bytes > 0 and neither; and -1
 * for a path that is no readable regular file. */
typedef struct mc_text_source {
    const char *text;              /* a host text of n_bytes (may be null when n_bytes == 0) ...                            */
    const char *path;              /* ... or, when not null, a regular file (text must be null; n_bytes is ignored: the file is sized) */
    int64_t n_bytes;
} mc_text_source;

/* ===== the per-site summary of a `.diffs.<k>` file on the GPU (make_bed.py:67-164 for BED, BED --control, BED --vo, GFF) =====
 * mc_bed_summarise: the text of the file (src) -> the bytes make_bed writes: rows whose context has 'M' at its centre, grouped
 * by the exact bytes of (chrom, pos, strand, context) in first-occurrence order, an entry written when depth >= min_depth and
 * (n_meth / depth >= mod_threshold) != control.  Integer counts, byte comparisons and one fp64 division: the bytes are the
 * reference's, or the call declines -- *status = 1, mc_last_error says why (and mc_bed_last_stats which line), nothing is
 * handed out and the caller runs the host code on the file.  Declined: a byte >= 0x80, a control byte other than tab and
 * newline (0x7f included), a line that is not 7 or 8 tab-separated fields (an empty line is one), a position that is not
 * 1-9 decimal digits, an empty context or label, a 7-field row with with_probs, a line longer than 65535 bytes, 2^31 - 2
 * lines or more, gff together with with_probs without site_stats, a text that does not fit into free device memory beside its
 * tables (the whole text stays resident).  *out points at n_out bytes of pinned memory owned by the context: valid until the next
 * mc_bed_summarise call on it or mc_bed_release.  Test knobs (environment): MCALLER_BED_HASH_MASK=<hex> is anded onto the 64-bit
 * hash of the key bytes; MCALLER_BED_TABLE_SLOTS=<n> fixes the number of table slots (fewer than 2 x the counted rows:
 * declined). */
typedef struct mc_bed_params {
    int64_t min_depth;             /* make_bed -d                                         */
    double mod_threshold;          /* make_bed -t                                         */
    int32_t control;               /* --control                                           */
    int32_t with_probs;            /* --vo                                                */
    int32_t gff;                   /* --gff                                               */
    int32_t site_stats;            /* gff && with_probs is made (below); 0: it declines   */
} mc_bed_params;
typedef struct mc_bed_stats {
    int64_t n_bytes, n_lines, n_counted, n_entries, n_sites, n_out_bytes;
    int64_t decline_line;          /* 0-based line the decline names, -1: none            */
    int32_t decline_reason;        /* 0: not declined; MC_BED_DECLINE_*                   */
    int32_t longest_probe;         /* slots a row looked at beyond its first, at most     */
    int64_t table_slots;
    int64_t kernel_bytes;          /* bytes the kernels read and wrote, by construction   */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_bed_stats;
#define MC_BED_DECLINE_HIGH_BYTE   1
#define MC_BED_DECLINE_CONTROL     2
#define MC_BED_DECLINE_FIELDS      3
#define MC_BED_DECLINE_POSITION    4
#define MC_BED_DECLINE_CONTEXT     5
#define MC_BED_DECLINE_LABEL       6
#define MC_BED_DECLINE_NO_PROB     7
#define MC_BED_DECLINE_LONG_LINE   8
#define MC_BED_DECLINE_TABLE       9
#define MC_BED_DECLINE_ROWS        10
#define MC_BED_DECLINE_MEMORY      11
#define MC_BED_DECLINE_OPTIONS     12
/* ... with a positions source; 13-15 name a line of the POSITIONS file, 16-19 a row, 20-25 an entry's first row */
#define MC_BED_DECLINE_POS_HIGH_BYTE 13  /* positions: a byte >= 0x80                                                  */
#define MC_BED_DECLINE_POS_CONTROL   14  /* positions: a control byte other than tab and newline                       */
#define MC_BED_DECLINE_POS_LONG_LINE 15  /* positions: a line longer than 65535 bytes                                  */
#define MC_BED_DECLINE_VALUE         16  /* a counted row with a value mc_decimal.h declines (nan, inf, blanks, ...)   */
#define MC_BED_DECLINE_FEW_VALUES    17  /* a counted row with fewer than two values                                   */
#define MC_BED_DECLINE_MANY_VALUES   18  /* a counted row with more than MC_BED_MAX_VALUES values                      */
#define MC_BED_DECLINE_VALUE_COUNT   19  /* a counted row with another number of values than the first counted row     */
#define MC_BED_DECLINE_ZERO_VARIANCE 20  /* depth >= 2 and a column without spread (the host prints inf / nan)         */
#define MC_BED_DECLINE_FAR_TAIL      21  /* a log10 p below -290                                                       */
#define MC_BED_DECLINE_PRINT_RANGE   22  /* a rounded value mc_rowtext.h does not print (|v| >= 1e9)                   */
#define MC_BED_DECLINE_ROUNDING_TIE  23  /* a value within its error bound of a rounding tie of np.round(., 3)         */
#define MC_BED_DECLINE_DEPTH         24  /* an entry of more than 100001 rows (the tail function's error is measured up to there) */
/* ... with site_stats or a FASTA source: 25-27 with --gff --vo (25 names a row, 26-27 an entry's first row); 28-30 name a line of the FASTA,
 * 31-32 an entry's first row */
#define MC_BED_DECLINE_PROBABILITY   25  /* a row of a written entry with a probability mc_decimal.h declines           */
#define MC_BED_DECLINE_STAT_RANGE    26  /* a fracLow / fracUp mc_rowtext.h does not print (0.0 and nan are printed)     */
#define MC_BED_DECLINE_QV_RANGE      27  /* |100 * mean| >= 2^53                                                        */
#define MC_BED_DECLINE_REF_HIGH_BYTE 28  /* FASTA: a byte >= 0x80                                                       */
#define MC_BED_DECLINE_REF_CONTROL   29  /* FASTA: a control byte other than tab and newline ('\r' too)                 */
#define MC_BED_DECLINE_REF_SEQ_BYTE  30  /* FASTA: a sequence line with a byte that is not a letter (the host strips blanks) */
#define MC_BED_DECLINE_REF_LETTER    31  /* an entry on '-' with a letter outside ACGTNM in its window (the host's KeyError) */
#define MC_BED_DECLINE_REF_CONTIG    32  /* a written entry whose contig the FASTA lacks (the host's KeyError)           */
#define MC_BED_MAX_VALUES 64
/* ... with make_bed -p: `positions` (null: none), a positions file beside the .diffs file (make_bed.py:13-19,:84-96,:115-127).
 * Every positions line with len(line) > 3, the newline counted, is stripped (blanks and tabs) and split on tabs; its first four fields are one tuple; a
 * row counts when its context has 'M' at its centre AND (chrom, pos text, decimal digits of pos + 1, strand) is such a tuple,
 * byte for byte.  Every entry is written (min_depth, mod_threshold and control select nothing).  A BED row gets two more
 * columns before the --vo list: str(np.round(., 3)) of the largest t statistic and of the sum of -log10 p of one-sample
 * t-tests of every value column of field 5 but the last against 0 (mcaller_amd/csrc/mc_tstat.h); "nan" twice at depth 1.
 * With gff the ordinary attributes are written for every entry.  Every printed value is the host's or the call declines
 * (MC_BED_DECLINE_* 13-24 on top of the above): the sums are compensated, the bound on |device - host| of every value is
 * derived (moments) and measured (tail function; profiles/tstat_error.json), and a value whose bound reaches a rounding
 * tie declines the file.  MCALLER_BED_HASH_MASK applies to the hash of the position tuples too.
 * ... with make_bed --gff --vo (site_stats) and --ref (`fasta`; null: none) (make_bed.py:36-48,:146-149).  gff && with_probs
 * with site_stats: every written entry carries ";fracLow=..;fracUp=..;identificationQv=.." from the probabilities of its rows in row order, in NumPy's own order of
 * additions (mcaller_amd/csrc/mc_npsum.h): the host's bits, no bound.  A FASTA: an entry's context in the GFF attributes is
 * the 41 bases around its position (Python's slice rule; upper-cased; complemented and reversed on '-'), a BED row keeps its own.
 * Declines on top of the above: MC_BED_DECLINE_* 25-32; a FASTA that does not fit beside the rest is MC_BED_DECLINE_MEMORY. */
int mc_bed_summarise(mc_ctx *ctx, const mc_text_source *src, const mc_text_source *positions, const mc_text_source *fasta,
                     const mc_bed_params *prm, const char **out, int64_t *n_out, int64_t *n_sites, int32_t *status);
int mc_bed_last_stats(mc_ctx *ctx, mc_bed_stats *out);
int mc_bed_release(mc_ctx *ctx);

/* ===== NumPy's summation order for make_bed --gff --vo (mcaller_amd/csrc/mc_npsum.h: one header for the host and the device) =====
 * p[0, n): an entry's probabilities in row order.  mc_gff_site_moments: out3 = {np.mean(p), np.var(p, ddof=1),
 * np.std(p, ddof=1) / np.sqrt(n)}, bit for bit.  mc_gff_site_stats: out3 = {frac - 2 se, frac + 2 se, 100 * mean}.  Both return
 * status bits: 1 fracLow / fracUp are nan (n = 1; printed), 2 a value the device does not print, 4 |100 * mean| >= 2^53, 8 the
 * workgroup's tree of additions differs from NumPy's recursion (never), 16 n < 1.  mc_gff_site_text: the attribute text the
 * kernels write, into buf -> its length (-1 - status bits: the device declines).  mc_gff_site_stats_device: the device build
 * on `count` arrays, one behind the other in p (off[count + 1]); out6 per array = {fracLow, fracUp, 100 * mean, mean, var, se}.
 * mc_npsum_se / mc_npsum_se_device: sqrt(var) / sqrt(n), both square roots correctly rounded. */
int mc_gff_site_moments(const double *p, int64_t n, double out3[3]);
int mc_gff_site_stats(const double *p, int64_t n, double frac, double out3[3]);
int mc_gff_site_text(const double *p, int64_t n, double frac, char *buf, int32_t cap);
int mc_gff_site_stats_device(mc_ctx *ctx, const double *p, const int64_t *off, const double *frac, int64_t count, double *out6,
                             int32_t *status);
double mc_npsum_se(double var, double n);
int mc_npsum_se_device(mc_ctx *ctx, const double *var, const double *n, int64_t count, double *se);

/* ===== the Student t arithmetic of make_bed -p (mcaller_amd/csrc/mc_tstat.h: one header for the host and the device) =====
 * mc_tstat: the host build on one triple (n rows, their mean, their sample variance with ddof = 1) -> status bits
 * (0: fine; 1: n < 2; 2: no spread or not finite; 4: log10 p < -290; 8: the continued fraction did not settle), *t the
 * statistic mean / sqrt(var / n), *log10_p the base-10 logarithm of the two-sided tail probability with n - 1 degrees of
 * freedom, computed in the log domain.  mc_tstat_device: the device build, a lane per triple.
 * mc_tstat_round3: rint(v * 1000) / 1000, the fp64 operations of np.round(v, 3).  mc_tstat_tie: 1 when np.round(h, 3) can
 * differ from np.round(v, 3) for an h within err of v (another thousandth, or the other zero).
 * mc_tstat_site: the host build of an entry's two printed values from its rows X[n_rows][n_cols] (row-major; the LAST
 * column is dropped, as make_bed drops the last value) -> out2 = {round3(max t), round3(sum -log10 p)}, the return value
 * the status bits above, 16: a rounding tie within the error bound, 32: more than 100001 rows, 64: a rounded value
 * mc_rowtext.h does not print. */
int mc_tstat(double n, double mean, double var, double *t, double *log10_p);
int mc_tstat_device(mc_ctx *ctx, const double *n, const double *mean, const double *var, int64_t count, double *t,
                    double *log10_p, int32_t *status);
double mc_tstat_round3(double v);
int mc_tstat_tie(double v, double err);
int mc_tstat_site(const double *X, int64_t n_rows, int32_t n_cols, double *out2);

/* ===== the hypergeometric tail of evaluate.py (mcaller_amd/csrc/mc_hypergeom.h: one header for the host and the device) =====
 * mc_hypergeom_tail: the host build on one case -> 0, or 1 for arguments outside 0 <= K <= N < 2^31, 0 <= d <= min(N, 2^20)
 * (*tail and *err NaN then); *tail = P(X >= k) for X the number of marked among d drawn without replacement from N of which K
 * are marked, *err a DERIVED bound on |*tail - exact| (0 where the tail is 1 or 0 by the range of X alone).
 * mc_hypergeom_tail_many: the same on `count` cases.  mc_hypergeom_tail_device: the device build, a lane per case.
 * mc_hypergeom_round4: rint(v * 10000) / 10000, the fp64 operations of np.round(v, 4).  mc_hypergeom_tie4: 1 when
 * np.round(h, 4) can differ from np.round(v, 4) for an h within err of v (another ten-thousandth, or the other zero). */
int mc_hypergeom_tail(int64_t N, int64_t K, int64_t d, int64_t k, double *tail, double *err);
int mc_hypergeom_tail_many(const int64_t *N, const int64_t *K, const int64_t *d, const int64_t *k, int64_t count, double *tail,
                           double *err);
int mc_hypergeom_tail_device(mc_ctx *ctx, const int64_t *N, const int64_t *K, const int64_t *d, const int64_t *k, int64_t count,
                             double *tail, double *err);
double mc_hypergeom_round4(double v);
int mc_hypergeom_tie4(double v, double err);
/* All 101 tails of one (N, K, d) in one call: x of 0 .. d passes c(x) = (100 x) / d + 1 of the thresholds j / 100, j = 0 .. 100
 * (x / d >= j / 100), so with mass102[c] = P(c(X) = c), c = 1 .. 101 (mass102[0] = 0: 102 doubles a case),
 * P(X >= k_min(d, j)) = sum over c > j of mass102[c].  *err: a DERIVED bound on the sum over c of |mass102[c] - exact|, which
 * bounds the error of every such tail; 0, with one mass of exactly 1, where X takes one value (d = N, K = 0, K = N).  Bad arguments
 * (as above): 1, NaN everywhere.  _many: `count` cases, 102 doubles each; _device: the device build, a lane per case. */
#define MC_HYPERGEOM_BUCKETS 102
int mc_hypergeom_masses(int64_t N, int64_t K, int64_t d, double *mass102, double *err);
int mc_hypergeom_masses_many(const int64_t *N, const int64_t *K, const int64_t *d, int64_t count, double *mass102, double *err);
int mc_hypergeom_masses_device(mc_ctx *ctx, const int64_t *N, const int64_t *K, const int64_t *d, int64_t count, double *mass102,
                               double *err);

/* ===== Fisher's exact test of compare_genomes --fisher (mcaller_amd/csrc/mc_fisher.h: one header for the host and the device) =====
 * The table of two samples' counts, K1 methylated reads of n1 and K2 of n2: X ~ Hypergeometric(n1 + n2, K1 + K2, n1), observed
 * K1; the two-sided p sums P(x) over the x with P(x) <= P(K1) (1 + 10^-7).  mc_fisher_exact: the host build on one table ->
 * *log10_p (0.0 exactly where X takes one value), *bound a DERIVED bound on |*log10_p - log10 of the exact rational p|, *status
 * the bits below (0: the value stands within its bound).  BAD_ARGS (not 0 <= K1 <= n1 <= 2^20, 0 <= K2 <= n2, n1 + n2 < 2^31):
 * NaN twice.  FAR_TAIL: log10 p < -250 -- the value and the bound still stand, unless K1's own mass lies below 2^-900 of the
 * mode's: -inf and +inf then.  SELECT: some P(x) / P(K1) lies within its own error of 1 + 10^-7, so the computed selection may
 * not be the exact one.  _many: `count` tables; _device: the device build, a lane per table.
 * mc_fisher_select(w, w_obs, steps): the selection predicate on two weights reached in at most `steps` steps from the mode:
 * bit 0 selected, bit 1 within the error. */
#define MC_FISHER_BAD_ARGS 1
#define MC_FISHER_FAR_TAIL 2
#define MC_FISHER_SELECT   4
int mc_fisher_exact(int64_t K1, int64_t n1, int64_t K2, int64_t n2, double *log10_p, double *bound, int32_t *status);
int mc_fisher_exact_many(const int64_t *K1, const int64_t *n1, const int64_t *K2, const int64_t *n2, int64_t count, double *log10_p,
                         double *bound, int32_t *status);
int mc_fisher_exact_device(mc_ctx *ctx, const int64_t *K1, const int64_t *n1, const int64_t *K2, const int64_t *n2, int64_t count,
                           double *log10_p, double *bound, int32_t *status);
int mc_fisher_select(double w, double w_obs, double steps);

/* ===== Benjamini-Hochberg q-values of compare_genomes --fdr, in the log domain (mcaller_amd/csrc/mc_bh.h) =====
 * L[n]: log10 p of the rows of one column (NaN: an untested row, which is not counted), bound[n]: the bound on each.  Q[n]:
 * log10 q, Q_(j) = min(0, min over k >= j of L_(k) + (log10 m - log10 k)) over the m tested rows sorted ascending; rounded[n]:
 * np.round(0.0 - Q, 3); NaN twice for an untested row.  *status: MC_BH_TIE when some row's value lies within the column's bound
 * (the largest of bound[], plus the derived slack of the terms) of a rounding tie; MC_BH_RANGE (NaN everywhere) for an L above
 * 0 or below -350 or a bound that is negative or not finite.  n <= 2^31 - 2.  mc_bh_adjust: the host build (a std::sort);
 * mc_bh_adjust_device: the kernels -- a device-wide radix sort of the rows' 64-bit keys, the terms, a two-level minimum from the
 * end, the finish at the rows' own places.  No floating-point atomic, and no atomic decides an order or a value. */
#define MC_BH_TIE   1
#define MC_BH_RANGE 2
int mc_bh_adjust(const double *L, const double *bound, int64_t n, double *Q, double *rounded, int32_t *status);
int mc_bh_adjust_device(mc_ctx *ctx, const double *L, const double *bound, int64_t n, double *Q, double *rounded, int32_t *status);

/* ===== the evaluation file of mcaller_amd/evaluate.py, made on the GPU (csrc/eval/mc_evalcalls.hip) =====
 * mc_eval_calls: the text of a `.diffs.<k>` file and of a labelled positions file -> the bytes evaluate.evaluate_calls gives for
 * them: the ROC tables by read, by site at min_depth or more, and by site at each of the n_depths subsampled depths (1 .. 16 of
 * them or none, each 1 .. 1024, strictly increasing: anything else is -12).  The integer tables are the host's bits; an expected
 * ("site d") value is printed only where its DERIVED bound shows that no value within the bound rounds to another ten-thousandth.
 * Otherwise, and wherever the host statement would raise or the device reader is not sure it reads what Python reads, the call
 * declines -- *status = 1, mc_last_error says why (mc_eval_last_stats: which file, line and reason), nothing is handed out and
 * the caller runs the host statement.  *out points at n_out bytes of pinned memory owned by the context: valid until the next
 * mc_eval_calls on it or mc_eval_release.  Test knobs (environment): MCALLER_EVAL_HASH_MASK=<hex> is anded onto the 64-bit hash
 * of a key; MCALLER_EVAL_TABLE_SLOTS=<n> fixes the number of slots of the truth table; MCALLER_EVAL_DEVICE_BYTES=<n> stands for
 * the free device memory. */
typedef struct mc_eval_params {
    int64_t min_depth;             /* least depth of a site of the "site all" table */
    int32_t n_depths;
    int32_t depths[16];
} mc_eval_params;
typedef struct mc_eval_stats {
    int64_t n_bytes, n_pos_bytes;  /* the two texts                                                       */
    int64_t n_rows, n_pos_lines;   /* lines of the .diffs text, of the positions text                     */
    int64_t n_kept, n_unlabelled, n_not_m;
    int64_t n_sites, n_pos_sites, n_neg_sites;     /* truth keys with a kept row                          */
    int64_t n_expect;              /* (site, depth) pairs the expectation ran on                          */
    int64_t decline_line;          /* 0-based line the decline names, -1: none                            */
    int64_t longest_probe;         /* slots a row's look-up read at the most                              */
    int64_t table_slots;
    int64_t kernel_bytes;          /* device memory the call held                                         */
    int32_t decline_reason;        /* 0: not declined; MC_EVAL_DECLINE_*                                  */
    int32_t decline_file;          /* 0: the .diffs text; 1: the positions text                           */
    double largest_bound;          /* the largest derived bound of a printed expected value (0: none)     */
    double ms_read, ms_h2d, ms_truth, ms_rows, ms_expect, ms_finish, ms_d2h, ms_total;
} mc_eval_stats;
#define MC_EVAL_DECLINE_HIGH_BYTE     1   /* a byte >= 0x80 (either file)                                                   */
#define MC_EVAL_DECLINE_CONTROL       2   /* a control byte other than tab and '\n' ('\r' too), or 0x7f                     */
#define MC_EVAL_DECLINE_LONG_LINE     3   /* a line of more than 65535 bytes                                                */
#define MC_EVAL_DECLINE_FIELDS        4   /* a .diffs line that is not eight tab-separated fields                           */
#define MC_EVAL_DECLINE_CONTEXT       5   /* an empty context                                                               */
#define MC_EVAL_DECLINE_POSITION      6   /* a position of a centre-M row that is not 1-18 decimal digits                   */
#define MC_EVAL_DECLINE_PROBABILITY   7   /* a kept row's probability that mc_decimal.h declines, or one outside [0, 1]     */
#define MC_EVAL_DECLINE_POS_TOKENS    8   /* a positions line of two or three tokens (the host's IndexError)                */
#define MC_EVAL_DECLINE_POS_NUMBER    9   /* a positions line whose second token is not 1-18 decimal digits                 */
#define MC_EVAL_DECLINE_TABLE         10  /* the truth table is full                                                        */
#define MC_EVAL_DECLINE_MEMORY        11  /* the texts do not fit into free device memory beside their tables               */
#define MC_EVAL_DECLINE_ROWS          12  /* 2^31 - 2 lines or more in a file                                               */
#define MC_EVAL_DECLINE_DEPTH         13  /* a site of 2^31 rows or more                                                    */
#define MC_EVAL_DECLINE_ROUNDING_TIE  14  /* an expected value whose bound reaches a tie of np.round(., 4)                  */
int mc_eval_calls(mc_ctx *ctx, const mc_text_source *diffs, const mc_text_source *positions, const mc_eval_params *params,
                  const char **out, int64_t *n_out, int32_t *status);
int mc_eval_last_stats(mc_ctx *ctx, mc_eval_stats *out);
int mc_eval_release(mc_ctx *ctx);

/* ===== decimal text -> double, correctly rounded (mcaller_amd/csrc/mc_decimal.h: one header for the host and the device) =====
 * float(s) of a token [+-]? digits? ('.' digits?)? ([eE] [+-]? digits)? with at least one mantissa digit whose significand
 * (leading zeros stripped, trailing zeros folded into the exponent) has at most 19 digits and whose decimal exponent q has
 * |q| <= 27; a zero significand is +-0.0 for any exponent.  Every other form float() accepts or rejects -- whitespace, '_',
 * inf, nan, more digits, other exponents, "", ".", "e5", "1e", hex -- is declined, never guessed.
 * mc_parse_double: the host build on s[0, n) -> 1: *out = float(s) bit for bit; 0: declined.
 * mc_parse_doubles_device: the device build, a lane per token: token i is text[off[i], off[i] + len[i]) (one outside
 * text[0, n_bytes) is declined); out[i] (0.0 where declined) and ok[i] as above. */
int mc_parse_double(const char *s, int32_t n, double *out);
int mc_parse_doubles_device(mc_ctx *ctx, const char *text, int64_t n_bytes, const int64_t *off, const int32_t *len, int64_t n,
                            double *out, uint8_t *ok);

/* ===== the rows of a `--training_tsv` file as matrices, made on the GPU (load_mCaller_data.py:14-29; csrc/train/mc_trainrows.hip) =====
 * The text of a `.diffs.<k>.train` file -> per label, in first-occurrence order, the fp64 feature rows and the contexts of the
 * rows tsv2matrix keeps (>= 6 comma-separated features, none the literal "0"), in file order.  A label is registered by the
 * first row that carries it, kept or not.  pairs[0, 2 * n_pairs): the two-character centre pairs a context may have (the keys
 * of base_models; at most MC_TRAINROWS_MAX_PAIRS).  The matrices are tsv2matrix's bit for bit, or the call declines --
 * *status = 1, mc_last_error says why (mc_train_rows_last_stats: which line and reason), the view is empty and the caller
 * runs the host code on the file.  Declined: MC_TRAINROWS_DECLINE_* below.  The view's pointers are memory owned by the
 * context: valid until the next mc_train_rows call on it or mc_train_rows_release.  Test knob (environment):
 * MCALLER_TRAINROWS_HASH_MASK=<hex> is anded onto the 64-bit hash of a label's bytes. */
#define MC_TRAINROWS_MAX_LABELS   16
#define MC_TRAINROWS_MAX_FEATURES 64
#define MC_TRAINROWS_MAX_CONTEXT  63
#define MC_TRAINROWS_MAX_PAIRS    32
typedef struct mc_train_rows_view {
    int32_t n_labels, n_features;  /* n_features: 0 when no row is kept                   */
    int32_t ctx_width, pad;        /* bytes per context: the longest kept one, NUL-padded */
    int64_t n_rows_total;
    const double *X;               /* [n_rows_total][n_features], the labels' blocks back to back, in label order */
    const char *contexts;          /* [n_rows_total][ctx_width]                           */
    const char *label_bytes;       /* label i = label_bytes[label_off[i], label_off[i + 1]) */
    int32_t label_off[MC_TRAINROWS_MAX_LABELS + 1];
    int32_t pad2;
    int64_t n_rows[MC_TRAINROWS_MAX_LABELS];
    int64_t first_line[MC_TRAINROWS_MAX_LABELS];      /* 0-based line that registered the label */
} mc_train_rows_view;
typedef struct mc_train_rows_stats {
    int64_t n_bytes, n_lines, n_kept;
    int64_t decline_line;          /* 0-based line the decline names, -1: none            */
    int32_t decline_reason;        /* 0: not declined; MC_TRAINROWS_DECLINE_*             */
    int32_t n_labels, n_features, in_place_blocks;    /* in_place_blocks: workgroups whose 256 lines did not fit the LDS stage */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_train_rows_stats;
#define MC_TRAINROWS_DECLINE_HIGH_BYTE     1   /* a byte >= 0x80                                                          */
#define MC_TRAINROWS_DECLINE_CONTROL       2   /* a control byte other than tab and newline (0x7f and '\r' included)       */
#define MC_TRAINROWS_DECLINE_FIELDS        3   /* a line with fewer than 7 tab-separated fields (the empty line is one)    */
#define MC_TRAINROWS_DECLINE_PAIR          4   /* a context whose centre pair is not among `pairs` (the host's KeyError)   */
#define MC_TRAINROWS_DECLINE_NUMBER        5   /* a kept row with a number mc_decimal.h declines                           */
#define MC_TRAINROWS_DECLINE_FEATURES      6   /* kept rows with differing feature counts, or more than 64 features        */
#define MC_TRAINROWS_DECLINE_CONTEXT       7   /* a context longer than 63 bytes                                           */
#define MC_TRAINROWS_DECLINE_LABELS        8   /* more than 16 distinct labels                                             */
#define MC_TRAINROWS_DECLINE_LONG_LINE     9   /* a line longer than 65535 bytes                                           */
#define MC_TRAINROWS_DECLINE_ROWS          10  /* 2^31 - 2 lines or more                                                   */
#define MC_TRAINROWS_DECLINE_MEMORY        11  /* the text does not fit into free device memory beside its outputs         */
int mc_train_rows(mc_ctx *ctx, const mc_text_source *src, const char *pairs, int32_t n_pairs, mc_train_rows_view *out,
                  int32_t *status);
int mc_train_rows_last_stats(mc_ctx *ctx, mc_train_rows_stats *out);
int mc_train_rows_release(mc_ctx *ctx);

/* ===== the merge behind `-t N` on the GPU: `sort -n -k2 | uniq` over the rows (mCaller.merge_like_sort_uniq; csrc/merge/mc_rowmerge.hip) =====
 * The lines of the part files (each with its '\n') -> every distinct line once, ordered by (numeric prefix of field 2 as
 * Decimal compares it, the bytes of the whole line, unsigned, the newline taking part): the bytes merge_like_sort_uniq
 * writes, or the call declines -- *status = 1, mc_last_error says why (mc_rows_merge_last_stats: which line, reason and
 * file), nothing is written and the caller runs the host code on the files.  Declined: MC_MERGE_DECLINE_* below.
 * mc_rows_merge_files writes to `<out_path>.merging` and renames it when complete; it removes no input.
 * mc_rows_merge_text takes one text; *out points at n_out bytes of pinned memory owned by the context: valid until the
 * next mc_rows_merge_* call on it or mc_rows_merge_release.
 * mc_sort_key: the numeric key of one line by the host build of mcaller_amd/csrc/mc_sortkey.h (needs no GPU) -> 0 and the key
 * (hi, lo), compared as one 128-bit unsigned number; 1: beyond 18 integer or 18 fraction digits; -12: bad arguments. */
typedef struct mc_rows_merge_stats {
    int64_t n_bytes, n_lines, n_lines_out, n_out_bytes;
    int64_t n_tied_after_key;      /* lines in a group of two or more once the numeric key is done */
    int32_t n_rounds;              /* rounds of 8 bytes the sort ran (the key's two words included)  */
    int32_t n_passes;              /* radix passes (8 bits each) that moved the rows               */
    int32_t largest_compared;      /* largest group finished by direct comparison                  */
    int32_t decline_reason;        /* 0: not declined; MC_MERGE_DECLINE_*                          */
    int64_t decline_line;          /* 0-based line (over all files) the decline names, -1: none    */
    int32_t decline_file, pad;     /* index of the part file it lies in, -1: none                  */
    int64_t kernel_bytes;          /* bytes the kernels read and wrote, by construction            */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_write, ms_total;
} mc_rows_merge_stats;
#define MC_MERGE_DECLINE_CR          1   /* a '\r' (bytes.splitlines cuts there)                                       */
#define MC_MERGE_DECLINE_NO_NEWLINE  2   /* a part file whose last byte is not '\n'                                    */
#define MC_MERGE_DECLINE_KEY         3   /* a numeric prefix with more than 18 integer or 18 fraction digits           */
#define MC_MERGE_DECLINE_LONG_LINE   4   /* a line longer than 65535 bytes                                             */
#define MC_MERGE_DECLINE_ROWS        5   /* 2^31 - 2 lines or more                                                     */
#define MC_MERGE_DECLINE_MEMORY      6   /* the texts do not fit into free device memory beside the output and tables  */
int mc_rows_merge_files(mc_ctx *ctx, const char *const *paths, int32_t n_paths, const char *out_path, int64_t *n_lines_out,
                        int32_t *status);
int mc_rows_merge_text(mc_ctx *ctx, const char *text, int64_t n_bytes, const char **out, int64_t *n_out, int32_t *status);
int mc_rows_merge_last_stats(mc_ctx *ctx, mc_rows_merge_stats *out);
int mc_rows_merge_release(mc_ctx *ctx);
int mc_sort_key(const char *line, int64_t n, uint64_t *hi, uint64_t *lo);

/* ===== the read qualities of a FASTQ file, made on the GPU (read_qual.py:15-47; csrc/mc_fastqrec.h, csrc/fastq/mc_fastqual.hip) =====
 * The text of a FASTQ file -> one (key, mean phred) pair per record in file order, in the layout of mc_fastq_view: the keys in
 * one pool with '\n' behind each, n + 1 offsets, n means.  The pairs are read_qual.extract_read_quality_py's bit for bit, or
 * the call declines -- *status = 1, mc_last_error says why (mc_fastq_quality_last_stats: which line and reason), the view is
 * empty and the caller runs the host reader on the file, which raises the reference's errors.  Declined:
 * MC_FASTQ_DECLINE_* below; of several offending lines the first is named, of several reasons on it the smallest.  The
 * view's pointers are pinned memory owned by the context: valid until the next mc_fastq_quality call on it or
 * mc_fastq_quality_release.
 * mc_fastq_records_host: the same rules (csrc/mc_fastqrec.h) run line by line on the CPU, no GPU and no context -> a handle
 * for mc_fastq_view / mc_fastq_free (null when declined); mc_fastq_records_host_decline: the line and reason of the calling
 * thread's last decline. */
typedef struct mc_fastq_quality_view {
    const char *key_pool;          /* key i = key_pool[key_off[i], key_off[i + 1] - 1), a '\n' behind it */
    const int64_t *key_off;        /* [n_records + 1] */
    const double *mean;            /* [n_records]; NaN for a record without bases */
    int64_t n_records;
} mc_fastq_quality_view;
typedef struct mc_fastq_quality_stats {
    int64_t n_bytes, n_lines, n_records;
    int64_t n_pieces;              /* pieces the quality lines were cut into: a wave sums one */
    int64_t decline_line;          /* 0-based line the decline names, -1: none            */
    int32_t decline_reason;        /* 0: not declined; MC_FASTQ_DECLINE_*                 */
    int32_t piece_bytes;           /* bytes of a piece                                    */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_fastq_quality_stats;
#define MC_FASTQ_DECLINE_HIGH_BYTE  1   /* a byte >= 0x80                                                                 */
#define MC_FASTQ_DECLINE_CONTROL    2   /* a control byte other than tab, '\n' and '\r', or 0x7f                          */
#define MC_FASTQ_DECLINE_LONE_CR    3   /* a '\r' not directly followed by '\n' (Python's universal newlines split there) */
#define MC_FASTQ_DECLINE_TITLE      4   /* a title line that does not start with '@' (a blank line between records too)   */
#define MC_FASTQ_DECLINE_PLUS       5   /* a third line that does not start with '+' (a file that ends inside a record)   */
#define MC_FASTQ_DECLINE_LENGTH     6   /* a quality line as long as its stripped sequence line it is not                 */
#define MC_FASTQ_DECLINE_EMPTY_ID   7   /* a title line with nothing but blanks and tabs behind its '@'                   */
#define MC_FASTQ_DECLINE_ROWS       8   /* 2^31 - 2 lines or more                                                         */
#define MC_FASTQ_DECLINE_MEMORY     9   /* the text does not fit into free device memory beside its outputs               */
#define MC_FASTQ_DECLINE_GZ         10  /* a path containing ".gz": decided by the caller (read_qual.py), nothing is read  */
int mc_fastq_quality(mc_ctx *ctx, const mc_text_source *src, mc_fastq_quality_view *out, int32_t *status);
int mc_fastq_quality_last_stats(mc_ctx *ctx, mc_fastq_quality_stats *out);
int mc_fastq_quality_release(mc_ctx *ctx);
int mc_fastq_records_host(const char *text, int64_t n_bytes, mc_fastq **out, int32_t *status);
int mc_fastq_records_host_decline(int32_t *reason, int64_t *line);

/* ===== two `make_bed --vo` BED files compared per site on the GPU (mcaller_amd/compare_genomes.py; csrc/mc_twosample.h,
 * csrc/compare/mc_bedcompare.hip) =====
 * mc_bed_compare: one row per key (chrom, start, end, strand) of bed1 that bed2 also has, in bed1's file order: the two samples' Mann-Whitney,
 * rank-sum, Student and Kolmogorov-Smirnov statistics and -log10 p values.  The bytes are those of
 * compare_genomes.compare_by_position, or the call declines -- *status = 1, mc_last_error says why (mc_bed_compare_last_stats:
 * which file, line and reason), nothing is handed out and the caller runs the host statement, which words the errors.
 * Declined: MC_CMP_DECLINE_* below; of several offending lines the first is named (bed1's before bed2's), of several reasons
 * on it the smallest.  *out points at n_out bytes of pinned memory owned by the context: valid until the next
 * mc_bed_compare call on it or mc_bed_compare_release.
 * mc_twosample: the arithmetic of one site by the host build of csrc/mc_twosample.h (needs no GPU) -> 0; out[9] = U, z_mwu, z_rs,
 * t, D, nlp_mwu, nlp_rs, nlp_t, nlp_ks (U and D as they are, the others rounded to three places), bound[9] the bound on
 * |device - host| of each before rounding, *status the TW_* bits of that header (0: every value is vouched for); -12: bad
 * arguments.  mc_twosample_device: the device build on k sites, site i = x[x_off[i], x_off[i + 1]) against y[y_off[i], y_off[i + 1])
 * -> out[k][9], bound[k][9], status[k].  mc_twosample_log10_2sf / _log10_kolmogorov: the two tail functions of the host build. */
typedef struct mc_cmp_stats {
    int64_t n_bytes1, n_bytes2, n_lines1, n_lines2;
    int64_t n_keys2;               /* bed2's lines in the table                                  */
    int64_t n_sites;               /* keys both files have                                       */
    int64_t n_values;              /* probabilities of the shared sites, both samples            */
    int64_t n_rank_small, n_rank_large;   /* sites a wave ranked (<= 64 pooled values), sites a workgroup ranked */
    int64_t n_out_bytes, table_slots;
    int64_t decline_line;          /* 0-based line in its file the decline names, -1: none       */
    int32_t decline_reason;        /* 0: not declined; MC_CMP_DECLINE_*                          */
    int32_t decline_file;          /* 1: bed1, 2: bed2, 0: none                                  */
    int32_t longest_probe;         /* slots the longest probe of the table looked at             */
    int32_t deepest_site;          /* pooled values of the deepest shared site                   */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
    int64_t n_fisher;              /* sites Fisher's test ran on (mc_bed_compare_with)           */
    int64_t n_fdr_columns;         /* columns of q-values made                                   */
    double ms_fdr;                 /* the sorts and minima of the q-values (part of ms_kernels)  */
} mc_cmp_stats;
#define MC_CMP_DECLINE_HIGH_BYTE   1   /* a byte >= 0x80                                                                  */
#define MC_CMP_DECLINE_CONTROL     2   /* a control byte other than tab and newline (0x7f and '\r' included)               */
#define MC_CMP_DECLINE_FIELDS      3   /* a line that does not have exactly 8 tab-separated fields (the host's ValueError) */
#define MC_CMP_DECLINE_EMPTY       4   /* an empty chrom, start, end or strand, or an empty probability list              */
#define MC_CMP_DECLINE_LONG_LINE   5   /* a line longer than 65535 bytes                                                  */
#define MC_CMP_DECLINE_ROWS        6   /* 2^31 - 2 lines or more in the two files together                                */
#define MC_CMP_DECLINE_MEMORY      7   /* the texts do not fit into free device memory beside their tables                */
#define MC_CMP_DECLINE_TABLE       8   /* the key table is full (MCALLER_CMP_TABLE_SLOTS)                                 */
#define MC_CMP_DECLINE_DUPLICATE   9   /* a key that occurs twice in one file (the host's dict rule does the file)        */
#define MC_CMP_DECLINE_NUMBER      10  /* a probability, on any line of either file, that mc_decimal.h declines            */
#define MC_CMP_DECLINE_DEPTH       11  /* a shared site with more than 8192 pooled values                                 */
#define MC_CMP_DECLINE_NAN         12  /* fewer than 3 pooled values or a zero pooled variance (SciPy's nan)              */
#define MC_CMP_DECLINE_ALL_EQUAL   13  /* all pooled values of a shared site equal (SciPy's nan)                          */
#define MC_CMP_DECLINE_FAR_TAIL    14  /* a log10 p below -290                                                            */
#define MC_CMP_DECLINE_PRINT       15  /* a value mc_rowtext.h does not print                                             */
#define MC_CMP_DECLINE_TIE         16  /* a value within its error bound of a rounding tie of np.round(., 3)              */
/* ----- two genomes with their own assemblies: the comparison through a Mauve alignment (csrc/compare/mc_xmfamap.inc; the
 * definition stands in mcaller_amd/compare_genomes.py) -----
 * mc_xmfa_map: the coordinate map of an XMFA file (src) for its sequence numbers seq1 (n1 bases in concatenated
 * coordinates, bed1's genome) and seq2 (n2 bases), built on the GPU and kept in the context until the next mc_xmfa_map call or
 * mc_xmfa_map_release: 8 bytes a base of genome 1.  view (may be NULL): host copies of g2[0 .. n1] and flip[0 .. n1], index g1,
 * 0: unmapped -- pinned memory of the context, valid as long as the map.  Declined (*status = 1, mc_last_error,
 * mc_xmfa_map_last_stats: reason and line; no map is kept): the MC_CMP_DECLINE_XMFA_* below, MC_CMP_DECLINE_ROWS,
 * MC_CMP_DECLINE_MEMORY (the map and the text beside free device memory, for which MCALLER_CMP_DEVICE_BYTES stands in tests).  Line by
 * line the first offending line is named and on it the smallest reason; in a file whose lines are sound, the header line of the
 * first offending entry and on it the smallest reason.
 * mc_bed_compare with contigs1 / contigs2 (both or neither, -12): the comparison through the resident map (-12 without one): a
 * bed1 line is matched to bed2 by its image, and a row carries the image's four fields behind bed1's.  contigs1 / contigs2: the
 * two genomes' .fai tables, whose totals must be the map's n1 and n2 (-12).  *n_unaligned (required with the tables, else may be
 * null): bed1's lines that have no image.  Declines as without the tables, and MC_CMP_DECLINE_LIFT_START. */
typedef struct mc_contig_table {
    int64_t n_contigs;
    const char *ids;               /* the names, one behind the other ...                          */
    const int64_t *id_off;         /* ... name i is ids[id_off[i], id_off[i + 1]); n_contigs + 1 entries */
    const int64_t *off;            /* contig i starts behind off[i] bases; n_contigs + 1 entries, off[n_contigs]: the genome's length */
} mc_contig_table;
typedef struct mc_xmfa_map_view {
    int64_t n1;
    const int64_t *g2;             /* [n1 + 1]                                                     */
    const uint8_t *flip;           /* [n1 + 1]                                                     */
} mc_xmfa_map_view;
typedef struct mc_xmfa_stats {
    int64_t n_bytes, n_lines;
    int64_t n_entries, n_blocks;   /* headers; '=' lines                                           */
    int64_t n_paired_blocks;       /* blocks that hold both sequence numbers, neither as 0-0       */
    int64_t n_columns;             /* columns of the paired blocks                                 */
    int64_t n_words;               /* 64-column words of one gap plane                             */
    int64_t n_mapped;              /* bases of genome 1 that have an image                         */
    int64_t n1, n2;
    int64_t decline_line;          /* 0-based line of the XMFA the decline names, -1: none         */
    int32_t decline_reason;        /* 0: not declined; MC_CMP_DECLINE_*                            */
    int32_t pad;
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_xmfa_stats;
#define MC_CMP_DECLINE_XMFA_BYTE     17  /* a '\r' or a byte >= 0x80 in the XMFA                                           */
#define MC_CMP_DECLINE_XMFA_HEADER   18  /* a malformed header, or a sequence line before its block's first header          */
#define MC_CMP_DECLINE_XMFA_SEQ_BYTE 19  /* a sequence byte that is neither '-' nor a letter                                */
#define MC_CMP_DECLINE_XMFA_COUNT    20  /* an entry whose non-gap count disagrees with its header                          */
#define MC_CMP_DECLINE_XMFA_COLUMNS  21  /* an entry with another column count than the entry before it in the block        */
#define MC_CMP_DECLINE_XMFA_UNCLOSED 22  /* an entry behind the last '='                                                    */
#define MC_CMP_DECLINE_XMFA_RANGE    23  /* an END beyond the .fai total of its genome                                      */
#define MC_CMP_DECLINE_XMFA_GENOME   24  /* a genome of more than 2^31 - 2 bases, or 2^31 columns or more in paired blocks  */
#define MC_CMP_DECLINE_LIFT_START    25  /* a bed1 start that is not plain digits (int() may accept it: the host decides)   */
/* ... with mc_bed_compare_with's options (compare_genomes --fisher --fdr; csrc/compare/mc_cmpfdr.inc).  fisher: one more column behind
 * nlp_ks, -log10 p of Fisher's exact test on the counts of the site's two lines (frac, field 5, is the count K over the line's n
 * probabilities: K = rint(frac n), sound iff 0 <= K <= n and K / n == frac in fp64).  fdr: behind that, -log10 of the
 * Benjamini-Hochberg q-value of each -log10 p column over the rows written (mc_bh_adjust below).  Null options, or both 0: mc_bed_compare,
 * byte for byte.  Declines on top of the above: 26-27, and MC_CMP_DECLINE_FAR_TAIL (Fisher's log10 p below -250), _TIE (a site's
 * nlp_fisher, or -- no line named -- a q-value within its column's bound of a rounding tie), _PRINT, _MEMORY (the sort buffers). */
#define MC_CMP_DECLINE_FRAC          26  /* a shared line whose frac mc_decimal.h declines or that is no count over its reads */
#define MC_CMP_DECLINE_FISHER_SELECT 27  /* a table with a mass within its error of the selection factor 1 + 10^-7           */
typedef struct mc_cmp_options {
    int32_t fisher, fdr;
} mc_cmp_options;
int mc_xmfa_map(mc_ctx *ctx, const mc_text_source *src, int32_t seq1, int32_t seq2, int64_t n1, int64_t n2, mc_xmfa_map_view *view,
                int32_t *status);
int mc_xmfa_map_last_stats(mc_ctx *ctx, mc_xmfa_stats *out);
int mc_xmfa_map_release(mc_ctx *ctx);
int mc_bed_compare(mc_ctx *ctx, const mc_text_source *bed1, const mc_text_source *bed2, const mc_contig_table *contigs1,
                   const mc_contig_table *contigs2, const char **out, int64_t *n_out, int64_t *n_sites, int64_t *n_unaligned,
                   int32_t *status);
int mc_bed_compare_with(mc_ctx *ctx, const mc_text_source *bed1, const mc_text_source *bed2, const mc_contig_table *contigs1,
                        const mc_contig_table *contigs2, const mc_cmp_options *opt, const char **out, int64_t *n_out, int64_t *n_sites,
                        int64_t *n_unaligned, int32_t *status);
int mc_bed_compare_last_stats(mc_ctx *ctx, mc_cmp_stats *out);
int mc_bed_compare_release(mc_ctx *ctx);
int mc_twosample(const double *x, int64_t n1, const double *y, int64_t n2, double *out, double *bound, int32_t *status);
int mc_twosample_device(mc_ctx *ctx, const double *x, const int64_t *x_off, const double *y, const int64_t *y_off, int64_t k,
                        double *out, double *bound, int32_t *status);
double mc_twosample_log10_2sf(double z);
double mc_twosample_log10_kolmogorov(double lam);

/* ===== a native sample against an unmodified control, site by site and without a model (mcaller_amd/compare_currents.py;
 * csrc/mc_curcombine.h, csrc/compare/mc_curcompare.inc) =====
 * mc_currents_compare: the two texts are the mCaller rows (.diffs, 7 or 8 fields) of the native sample and of the control.  One row per
 * key (chrom, pos, strand) of the native text that the control has too, with at least opt->depth rows in both, in the order of the
 * keys' first native rows: per value column Student's t, then per test (Mann-Whitney, rank-sum, Student, Kolmogorov-Smirnov) the
 * Bonferroni combination of the columns' -log10 p; opt->fdr: behind them the Benjamini-Hochberg q-values (mc_bh_adjust) of the four.
 * opt->by (0 .. 3: mwu, rs, t, ks; -1: none): the rows whose printed value of that test (with fdr: its q-value) is at least
 * opt->threshold also go to res->bed as BED lines.  opt->n_columns is c, the values of a row less the read quality, and opt->log10c the
 * caller's float(np.log10(c)): no side computes it anew.  The bytes are those of compare_currents.compare_currents, or the call
 * declines -- *status = 1, mc_last_error says why (mc_currents_compare_last_stats: which file, line and reason), nothing is handed out
 * and the caller runs the host statement, which words the errors.  Declines: MC_CMP_DECLINE_* above where they apply, and 28-30.
 * res->out and res->bed point at pinned memory owned by the context: valid until the next mc_currents_compare call on it or
 * mc_currents_compare_release.
 * mc_curcombine: one test's c columns by the host build of csrc/mc_curcombine.h (needs no GPU) -> 0; out2 = the combined log10 p
 * before rounding and np.round(0.0 - L, 3), *bound_out the bound on |device L - host L|, *status the CC_* bits of that header
 * (0: the value is vouched for); -12: bad arguments. */
#define MC_CMP_DECLINE_CUR_FIELDS    28  /* a line that does not have 7 or 8 tab-separated fields (the host's ValueError)      */
#define MC_CMP_DECLINE_CUR_VALUES    29  /* a line whose number of values is not n_columns + 1, or fewer than 2               */
#define MC_CMP_DECLINE_CUR_POS       30  /* a pos that is not 1 .. 9 plain digits (int() may accept it: the host decides)     */
typedef struct mc_cur_options {
    int32_t depth, fdr, by, n_columns;
    double threshold, log10c;
} mc_cur_options;
typedef struct mc_cur_result {
    const char *out, *bed;
    int64_t n_out, n_bed, n_sites, n_sig;
} mc_cur_result;
typedef struct mc_cur_stats {
    int64_t n_bytes1, n_bytes2, n_lines1, n_lines2;
    int64_t n_keys;                /* keys of the two files together                             */
    int64_t n_sites, n_columns;    /* kept sites; value columns of a row                         */
    int64_t n_values;              /* numbers of the kept sites' rows, both samples              */
    int64_t n_rank_small, n_rank_large;   /* (site, column) pairs a wave ranked (<= 64 pooled values), a workgroup ranked */
    int64_t n_out_bytes, n_bed_bytes, n_sig, table_slots;
    int64_t decline_line;          /* 0-based line in its file the decline names, -1: none       */
    int32_t decline_reason;        /* 0: not declined; MC_CMP_DECLINE_*                          */
    int32_t decline_file;          /* 1: native, 2: control, 0: none                             */
    int32_t longest_probe;         /* slots the longest probe of the table looked at             */
    int32_t deepest_site;          /* pooled rows of the deepest kept site                       */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
    int64_t n_fdr_columns;         /* columns of q-values made                                   */
    double ms_fdr;                 /* the sorts and minima of the q-values (part of ms_kernels)  */
} mc_cur_stats;
int mc_currents_compare(mc_ctx *ctx, const mc_text_source *native, const mc_text_source *control, const mc_cur_options *opt,
                        mc_cur_result *res, int32_t *status);
int mc_currents_compare_last_stats(mc_ctx *ctx, mc_cur_stats *out);
int mc_currents_compare_release(mc_ctx *ctx);
int mc_curcombine(const double *L, const double *bound, int64_t c, double log10c, double out2[2], double *bound_out, int32_t *status);

/* ===== the rows of every site split in two by their currents (mcaller_amd/cluster_sites.py; csrc/mc_linkage.h,
 * csrc/compare/mc_sitecluster.inc) =====
 * mc_sites_cluster: the text is the mCaller rows (.diffs, 7 or 8 fields) of one sample.  One row per key (chrom, pos, strand) with at
 * least opt->depth usable rows among its first opt->max_depth, in the order of the keys' first rows: the rows' vectors (opt->n_columns
 * values, the read quality left out) linked by complete linkage under opt->metric down to two clusters, the clusters' sizes and
 * methylated rows, the heights h_top and h_sub and the adjusted Rand index of (cluster, label).  opt->mixed: the rows with
 * min(n_1, n_2) / (n_1 + n_2) >= opt->min_minor and h_top >= opt->min_gap * h_sub also go to res->bed as BED lines.  The bytes are
 * those of cluster_sites.cluster_sites, or the call declines -- *status = 1, mc_last_error says why (mc_sites_cluster_last_stats:
 * line and reason), nothing is handed out and the caller runs the host statement, which words the errors.  Declines:
 * MC_CMP_DECLINE_HIGH_BYTE, _CONTROL, _LONG_LINE, _ROWS, _MEMORY, _TABLE, _NUMBER, _PRINT (a height outside mc_rowtext.h's range) and
 * the three _CUR_* (fewer than 2 columns is _CUR_VALUES at line 0).  A depth is never a decline.  No code for a value that is not finite:
 * mc_decimal.h hands out no such value, it declines the token (_NUMBER).
 * res->out and res->bed point at pinned memory owned by the context: valid until the next mc_sites_cluster call on it or
 * mc_sites_cluster_release.  Test knobs as for mc_currents_compare (MCALLER_CMP_HASH_MASK, _TABLE_SLOTS, _DEVICE_BYTES).
 * mc_site_cluster_host: one site by the host build of csrc/mc_linkage.h (needs no GPU): values[n, c] row-major, n <= 1024, metric
 * MC_CLU_* -> 0: labels_out[i] = 0 (a flat row), 1 or 2, out3 = h_top, h_sub, the usable rows; 1: fewer than 2 usable rows (out3[2]
 * alone is set); -12: bad arguments.  mc_site_ari_host: the adjusted Rand index from the clusters' sizes and methylated rows. */
#define MC_CLU_CORRELATION 0
#define MC_CLU_EUCLIDEAN   1
#define MC_CLU_MAX_DEPTH   1024
#define MC_CLU_WAVE_ROWS   64    /* up to here a wave links a site (kl_link_small)                       */
#define MC_CLU_LDS_ROWS    141   /* up to here a workgroup keeps the distance matrix in LDS, beyond in its slab of device memory */
typedef struct mc_clu_options {
    int32_t depth, max_depth, metric, mixed, n_columns, pad;
    double min_minor, min_gap;
} mc_clu_options;
typedef struct mc_clu_result {
    const char *out, *bed;
    int64_t n_out, n_bed, n_sites, n_mixed;
} mc_clu_result;
typedef struct mc_clu_stats {
    int64_t n_bytes, n_lines, n_keys;
    int64_t n_candidates;          /* keys with at least depth rows                               */
    int64_t n_sites, n_mixed;      /* kept sites; those in the bed                                */
    int64_t n_rows;                /* rows of the candidates                                      */
    int64_t n_link_small, n_link_lds, n_link_slab;   /* kept sites by the kernel that linked them */
    int64_t slab_groups, slab_bytes;                 /* persistent workgroups of the slab kernel, bytes of their slabs */
    int64_t n_out_bytes, n_bed_bytes, table_slots;
    int64_t decline_line;          /* 0-based line the decline names, -1: none                    */
    int32_t decline_reason;        /* 0: not declined; MC_CMP_DECLINE_*                           */
    int32_t longest_probe;         /* slots the longest probe of the table looked at              */
    int32_t deepest_site;          /* usable rows of the deepest kept site                        */
    int32_t n_columns;
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_clu_stats;
int mc_sites_cluster(mc_ctx *ctx, const mc_text_source *source, const mc_clu_options *opt, mc_clu_result *res, int32_t *status);
int mc_sites_cluster_last_stats(mc_ctx *ctx, mc_clu_stats *out);
int mc_sites_cluster_release(mc_ctx *ctx);
int mc_site_cluster_host(const double *values, int64_t n, int64_t c, int32_t metric, int32_t *labels_out, double out3[3]);
double mc_site_ari_host(int64_t n1, int64_t n2, int64_t m1, int64_t m2);

/* ===== methylation linkage between sites along reads (mcaller_amd/phase_reads.py; csrc/mc_pairphase.h,
 * csrc/compare/mc_readphase.inc) =====
 * mc_reads_phase: the text is the mCaller rows (.diffs, 7 or 8 fields) of one sample.  A site (chrom, pos, strand) is kept with at
 * least opt->depth rows; for every pair of kept sites of one chrom and strand at most opt->max_dist apart, the reads (chrom, read,
 * strand) with a row at both are counted by (A methylated, B methylated).  res->out: one row per pair with at least opt->min_reads
 * shared reads and every margin at least opt->min_margin -- the counts, phi, -log10 of Fisher's p and, with opt->fdr, of its
 * Benjamini-Hochberg q -- ordered by A's first row, then B's pos; res->reads: one row per read with a row at a kept site, in the
 * order of the reads' first rows; res->bed (opt->bed): the kept sites that are A or B of a written pair whose printed value (fdr:
 * the q-value) is at least opt->threshold, as BED lines.  opt->n_columns: the values of a row less the read quality.  The bytes are
 * those of phase_reads.phase_reads, or the call declines -- *status = 1, mc_last_error says why (mc_reads_phase_last_stats: line and
 * reason), nothing is handed out and the caller runs the host statement, which words the errors.  Declines: MC_CMP_DECLINE_HIGH_BYTE,
 * _CONTROL, _LONG_LINE, _ROWS, _MEMORY (the text, its tables, the S W pair counters of 8 bytes and their columns, the sort buffers),
 * _TABLE (the site table, the read table or the strands'), _NUMBER, the three _CUR_* (no value column is _CUR_VALUES at line 0),
 * _DUPLICATE (a read with two rows at one pos: the later line), _DEPTH (a kept site of more than MC_PHASE_MAX_DEPTH rows: the four
 * counts of a pair are 16-bit fields of one word), _FAR_TAIL, _FISHER_SELECT, _TIE, _PRINT (Fisher's value of a written pair: site
 * A's first line; a q-value's tie names no line) and MC_CMP_DECLINE_READ_ROWS.  A file without a kept site hands out nothing.
 * The three outputs point at pinned memory owned by the context: valid until the next mc_reads_phase call on it or
 * mc_reads_phase_release.  Test knobs as for mc_currents_compare: MCALLER_CMP_HASH_MASK and MCALLER_CMP_TABLE_SLOTS hold for the read
 * table too, MCALLER_CMP_DEVICE_BYTES for the counters and the sort buffers too.
 * mc_pair_phi: phi of one table by the host build of csrc/mc_pairphase.h (needs no GPU) and np.round(phi, 3) -> 0; 1: a margin of
 * zero, nothing is written; -12: bad arguments (a count below 0 or above 65535). */
#define MC_CMP_DECLINE_READ_ROWS     31  /* a read (chrom, read, strand) with more than MC_PHASE_GROUP_ROWS rows              */
#define MC_PHASE_WAVE_ROWS   64      /* up to here a wave orders a read's rows (kr_order)                    */
#define MC_PHASE_GROUP_ROWS  2048    /* up to here a workgroup does, in LDS; beyond, the file is declined    */
#define MC_PHASE_MAX_DEPTH   65535   /* rows of a kept site                                                  */
typedef struct mc_phase_options {
    int32_t depth, max_dist, min_reads, min_margin, fdr, bed, n_columns, pad;
    double threshold;
} mc_phase_options;
typedef struct mc_phase_result {
    const char *out, *reads, *bed;
    int64_t n_out, n_reads_bytes, n_bed, n_pairs, n_reads, n_linked;
} mc_phase_result;
typedef struct mc_phase_stats {
    int64_t n_bytes, n_lines, n_keys;
    int64_t n_sites;               /* kept sites                                                  */
    int64_t n_read_keys;           /* reads (chrom, read, strand) of the file                     */
    int64_t n_reads_wave, n_reads_group;   /* reads whose rows a wave ordered (<= 64 rows), a workgroup ordered */
    int64_t window;                /* W: the most kept sites behind a site within max_dist, at least 1 */
    int64_t n_counters;            /* n_sites * window                                            */
    int64_t n_instances;           /* pair instances counted: atomics of the hot path             */
    int64_t n_pairs, n_reads, n_linked;    /* rows written, rows of the reads output, lines of the bed */
    int64_t n_out_bytes, n_reads_bytes, n_bed_bytes, table_slots, read_table_slots;
    int64_t decline_line;          /* 0-based line the decline names, -1: none                    */
    int32_t decline_reason;        /* 0: not declined; MC_CMP_DECLINE_*                           */
    int32_t longest_probe, longest_read_probe;   /* slots the longest probe of the site table, the read table looked at */
    int32_t deepest_site;          /* rows of the deepest kept site                               */
    int32_t longest_read;          /* rows of the longest read                                    */
    int32_t n_columns;
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_phase_stats;
int mc_reads_phase(mc_ctx *ctx, const mc_text_source *source, const mc_phase_options *opt, mc_phase_result *res, int32_t *status);
int mc_reads_phase_last_stats(mc_ctx *ctx, mc_phase_stats *out);
int mc_reads_phase_release(mc_ctx *ctx);
int mc_pair_phi(int64_t n11, int64_t n10, int64_t n01, int64_t n00, double *phi, double *rounded);

/* ===== methylated motifs found de novo from called sites on the GPU (mcaller_amd/find_motifs.py; csrc/motifs/mc_motifscan.hip) =====
 * mc_motif_report, with iupac = 0 and max_motifs = 0.  For every shape (a string of X and '.', first and last X, at most MC_MOTIF_MAX_WIDTH wide, 2 to 8 X), every X of it as the called
 * letter and every assignment of A, C, G, T to the X: the candidates of the reference (ref: contig_len, seq_off and the upper-cased
 * seq; the masks are not read) that stand in such a window, those the bed or the control lists (covered; without a control all
 * are) and those the bed lists (methylated).  The rows with nMethylated >= min_sites and nMethylated / nCovered >= min_fraction,
 * less (keep_all = 0) those a selected row on a strict subset of their letters explains, ordered and printed as
 * find_motifs.find_motifs does -- or the call declines: *status = 1, mc_last_error says why (mc_motif_report_last_stats: which
 * file, line and reason), nothing is handed out and the caller runs the host statement, which words the errors.  Of several
 * offending lines the first is named (the bed's before the control's), of several reasons on it the smallest.  *out points at
 * n_out bytes of pinned memory owned by the context: valid until the next mc_motif_report call on it or mc_motif_report_release.
 * Test knobs, read per call: MCALLER_MOTIF_HASH_MASK=<hex>, MCALLER_MOTIF_TABLE_SLOTS=n (the contig table),
 * MCALLER_MOTIF_STRETCH=n (bases a workgroup of the counting kernel takes: a multiple of 64, the effective value is in the
 * stats), MCALLER_MOTIF_DEVICE_BYTES=n (stands for the free device memory), MCALLER_TEXT_STAGE_BYTES (the feed). */
#define MC_MOTIF_MAX_SHAPES 64
#define MC_MOTIF_MAX_WIDTH 24
typedef struct mc_motif_params {
    int32_t base;                  /* 'A', 'C', 'G' or 'T'                                        */
    int32_t n_shapes;              /* 1 .. MC_MOTIF_MAX_SHAPES                                    */
    char shapes[MC_MOTIF_MAX_SHAPES][MC_MOTIF_MAX_WIDTH + 8];      /* NUL-terminated              */
    int64_t min_sites;
    double min_fraction;
    int32_t keep_all, pad;         /* --all: rows that a shorter selected row explains stay       */
    const char *contig_ids;        /* the ids of ref's contigs, one behind the other ...          */
    const int64_t *contig_id_off;  /* ... id i is contig_ids[contig_id_off[i], contig_id_off[i + 1]); n_contigs + 1 entries */
} mc_motif_params;
typedef struct mc_motif_stats {
    int64_t n_bytes1, n_bytes2, n_lines1, n_lines2;
    int64_t n_candidates;          /* (position, strand) pairs whose base is the called base     */
    int64_t n_sites, n_control;    /* distinct sites the bed lists, the control lists            */
    int64_t n_off_base;            /* distinct listed sites whose base is not the called base    */
    int64_t n_selected, n_rows;    /* entries over both thresholds; rows after redundancy        */
    int64_t stretch, n_stretches;  /* bases a workgroup of km_count takes (effective), workgroups per table */
    int64_t n_entries, table_slots, n_out_bytes;
    int64_t decline_line;          /* 0-based line in its file the decline names, -1: none       */
    int32_t decline_reason;        /* 0: not declined; MC_MOTIF_DECLINE_*                        */
    int32_t decline_file;          /* 1: the bed, 2: the control, 0: none                        */
    int32_t n_tables_lds, n_tables_global;      /* (shape, j) tables counted in LDS, straight in global memory */
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
} mc_motif_stats;
#define MC_MOTIF_DECLINE_HIGH_BYTE   1   /* a byte >= 0x80                                                          */
#define MC_MOTIF_DECLINE_CONTROL     2   /* a control byte other than tab and newline (0x7f and '\r' included)       */
#define MC_MOTIF_DECLINE_LONG_LINE   3   /* a line longer than 65535 bytes                                          */
#define MC_MOTIF_DECLINE_FIELDS      4   /* a line with fewer than 6 tab-separated fields (the host's ValueError)   */
#define MC_MOTIF_DECLINE_FIELD       5   /* an empty chrom, a start that is not plain digits, a strand other than + / - */
#define MC_MOTIF_DECLINE_CHROM       6   /* a chrom that is no contig of the reference                              */
#define MC_MOTIF_DECLINE_RANGE       7   /* a start outside its contig                                              */
#define MC_MOTIF_DECLINE_TABLE       8   /* the contig table is full (MCALLER_MOTIF_TABLE_SLOTS)                    */
#define MC_MOTIF_DECLINE_MEMORY      9   /* the reference, the texts and the tables do not fit into device memory   */
#define MC_MOTIF_DECLINE_REFERENCE   10  /* a reference of 2^31 bases or more (the counters are 32-bit)             */
#define MC_MOTIF_DECLINE_PRINT       11  /* a fraction mc_rowtext.h does not print                                  */
#define MC_MOTIF_DECLINE_ROWS        12  /* 2^31 - 2 lines or more in the two files together                        */
int mc_motif_report_last_stats(mc_ctx *ctx, mc_motif_stats *out);
/* iupac != 0, --iupac: the rows merged into degenerate motifs (the definition: mcaller_amd/find_motifs.py; csrc/motifs/mc_motifiupac.inc).  The
 * same declines and ownership of *out as above; a row is a maximal pure pattern, SPEC carries IUPAC letters.  Every
 * table's purity lattice (15^(k-1) bytes) is resident during the call: lattice_bytes is what that adds to the plain call's need,
 * counted against free device memory (MCALLER_MOTIF_DEVICE_BYTES) before anything is allocated -> MC_MOTIF_DECLINE_MEMORY.
 * mc_motif_report_last_stats holds for these calls too (n_selected: maximal patterns over both thresholds). */
typedef struct mc_motif_iupac_stats {
    int64_t n_good;                /* concrete entries seen covered with nMethylated / nCovered >= min_fraction */
    int64_t n_pure, n_maximal;     /* patterns whose members are all good; those no larger pure pattern holds   */
    int64_t lattice_bytes;         /* good flags, lattices and the transform's two scratch blocks               */
    int64_t decline_line;          /* as in mc_motif_stats                                                      */
    int32_t decline_reason, decline_file;
} mc_motif_iupac_stats;
int mc_motif_report_iupac_last_stats(mc_ctx *ctx, mc_motif_iupac_stats *out);
/* max_motifs != 0, --iterative: the motifs peeled off one at a time (the definition: mcaller_amd/find_motifs.py;
 * csrc/motifs/mc_motifiter.inc).  The same declines and ownership of *out as above; iupac (0: concrete rows, else degenerate ones),
 * max_motifs 1 .. MC_MOTIF_MAX_ROUNDS (0: not iterative; anything else: -12).  Round 1 is the call with max_motifs = 0; every later round takes the candidates the printed row explains out of the
 * candidate planes and out of every table's counters and selects again: planes, tables and lattices stay on the device for the
 * whole call.  The list of a round's explained candidates (list_bytes: 8 bytes a base) is counted against free device memory
 * (MCALLER_MOTIF_DEVICE_BYTES) before anything is allocated -> MC_MOTIF_DECLINE_MEMORY.  mc_motif_report_last_stats and
 * mc_motif_report_iupac_last_stats hold the figures of round 1 (n_rows and n_out_bytes: of what is handed out). */
#define MC_MOTIF_MAX_ROUNDS 64
typedef struct mc_motif_iter_stats {
    int64_t n_rounds;              /* rows printed                                                              */
    int64_t n_explained[MC_MOTIF_MAX_ROUNDS];      /* candidates row r explains: its nGenome                    */
    int64_t n_unexplained;         /* methylated candidates left after the last round                           */
    int64_t list_bytes;            /* the list of a round's explained candidates                                */
    int64_t need_bytes;            /* all the call counted against free device memory before it allocated       */
    int64_t decline_line;          /* as in mc_motif_stats                                                      */
    int32_t decline_reason, decline_file;
    double ms_first_round;         /* from the first kernel to the first row: the plain call's ms_kernels       */
    double ms_later_rounds;        /* all later rounds together, the explain step of the round before included  */
} mc_motif_iter_stats;
int mc_motif_report(mc_ctx *ctx, const mc_ref_view *ref, const mc_text_source *bed, const mc_text_source *control_or_null,
                    const mc_motif_params *params, int32_t iupac, int32_t max_motifs, const char **out, int64_t *n_out, int64_t *n_rows,
                    int32_t *status);
int mc_motif_report_iter_last_stats(mc_ctx *ctx, mc_motif_iter_stats *out);
/* The methylated candidates the last iterative mc_motif_report call left unexplained, as two bit planes of n_words 64-bit words in
 * pinned memory owned by the context ('+' and '-'; bit i of word w: base index 64 w + i), and contig_start[c], the base index of
 * contig c's first base (n_contigs entries).  Valid until the next mc_motif_report call; all null / 0 after a decline. */
int mc_motif_report_iter_left(mc_ctx *ctx, const uint64_t **plus, const uint64_t **minus, int64_t *n_words, const int64_t **contig_start,
                              int32_t *n_contigs);
int mc_motif_report_release(mc_ctx *ctx);

/* ===== motif methylation per contig or window and every bin's nearest bins (mcaller_amd/motif_profile.py;
 * csrc/motifs/mc_motifprofile.inc) =====
 * For 1 .. MC_PROFILE_MAX_MOTIFS motifs (upper-case IUPAC letters, bit j of called[i]: letter j of motif i is a called letter and
 * holds the base; the rule: csrc/mc_iupac.h) and every bin -- a contig of ref (window 0), or a window of `window` >= 64 bases of
 * one -- the sites of the motif, those the bed or the control lists (without a control: all) and those the bed lists; one line per
 * (bin, motif) with a site, as motif_profile.motif_profile writes it.  neighbours 1 .. MC_PROFILE_MAX_NEIGHBOURS (0: none): for
 * every bin with a defined motif (nCovered >= min_sites) its nearest bins by the mean absolute difference of the fractions over the
 * motifs both define (at least min_shared), as the definition's second file.  ref, the sources, the ids and the declines
 * (MC_MOTIF_DECLINE_*; *status = 1, mc_last_error, the stats name file, line and reason) are mc_motif_report's, and so are the test
 * knobs MCALLER_MOTIF_HASH_MASK, MCALLER_MOTIF_TABLE_SLOTS and MCALLER_MOTIF_DEVICE_BYTES: all the call needs before the texts'
 * line starts and the two outputs (need_bytes) is counted against free device memory before anything is allocated.  The result's
 * blocks are pinned memory owned by the context: valid until the next mc_motif_profile call on it or mc_motif_profile_release. */
#define MC_PROFILE_MAX_MOTIFS 64
#define MC_PROFILE_MAX_NEIGHBOURS 16
typedef struct mc_motif_profile_params {
    int32_t base;                  /* 'A', 'C', 'G' or 'T'                                        */
    int32_t n_motifs;              /* 1 .. MC_PROFILE_MAX_MOTIFS                                  */
    const char *letters;           /* the motifs' letters, one motif behind the other ...         */
    const int64_t *letters_off;    /* ... motif i is letters[letters_off[i], letters_off[i + 1]); n_motifs + 1 entries */
    const uint32_t *called;        /* n_motifs masks                                              */
    const char *specs;             /* what a row prints for motif i (its canonical text): specs[spec_off[i], spec_off[i + 1]) */
    const int64_t *spec_off;
    int64_t window;                /* 0: a bin is a contig; else >= 64                            */
    int64_t min_sites;             /* >= 1                                                        */
    int32_t neighbours;            /* 0: no second file; else 1 .. MC_PROFILE_MAX_NEIGHBOURS      */
    int32_t min_shared;            /* >= 1                                                        */
    const char *contig_ids;        /* as in mc_motif_params                                       */
    const int64_t *contig_id_off;
} mc_motif_profile_params;
typedef struct mc_motif_profile_result {
    const char *out;               /* the profile file                                            */
    int64_t n_out, n_rows;
    const char *nn;                /* the neighbours file                                         */
    int64_t n_nn, n_nn_rows;
} mc_motif_profile_result;
typedef struct mc_motif_profile_stats {
    int64_t n_bytes1, n_bytes2, n_lines1, n_lines2;
    int64_t n_candidates, n_sites, n_control, n_off_base;     /* as in mc_motif_stats                  */
    int64_t n_bins, n_rows;        /* bins; lines of the profile file                             */
    int64_t n_defined;             /* bins with at least one defined motif                        */
    int64_t n_pairs;               /* ordered pairs of bins that have a distance (0 without neighbours) */
    int64_t n_nn_rows;             /* lines of the neighbours file                                */
    int64_t table_slots, need_bytes, n_out_bytes, n_nn_bytes;
    int64_t nn_lds_bytes;          /* dynamic LDS of a workgroup of the neighbours kernel         */
    int64_t decline_line;          /* as in mc_motif_stats                                        */
    int32_t decline_reason, decline_file;
    double ms_read, ms_h2d, ms_kernels, ms_d2h, ms_total;
    double ms_counts;              /* of ms_kernels: from the first launch until the profile file's sizes are known */
    double ms_neighbours;          /* of ms_kernels: the neighbours kernel, waited for            */
} mc_motif_profile_stats;
int mc_motif_profile(mc_ctx *ctx, const mc_ref_view *ref, const mc_text_source *bed, const mc_text_source *control_or_null,
                     const mc_motif_profile_params *params, mc_motif_profile_result *result, int32_t *status);
int mc_motif_profile_last_stats(mc_ctx *ctx, mc_motif_profile_stats *out);
int mc_motif_profile_release(mc_ctx *ctx);

/* ===== measurement plumbing: a table as nanopolish-eventalign text (13 columns), written by all host cores =====
 * For file-to-file timing on synthetic workloads (bench.py); seq = the contig's bases (k-mers of columns 3 and 10). */
int mc_synth_write_tsv(const char *path, const mc_table_view *table, const char *seq, int64_t seq_len, const char *contig,
                       const char *const *read_names, int32_t n_threads, int64_t *n_bytes);

#ifdef __cplusplus
}
#endif
#endif
