// mc_ctx.h -- the context of libmcaller_hip.so as its host units see it (mc_stream.hip: the passes; mc_tables.hip: table slots, the
// device parser's host side, the reference; mc_context.hip: life cycle and classifier setters; mc_rowtext_host.hip: rows of text;
// mc_comm.hip: RCCL), and the few functions that cross those units.  Included by them and by nothing else.  Everything the context
// takes from the runtime is held by an owner of mc_own.h: nothing here is freed by hand.  What the file pipelines keep between
// calls (mc_textfeed.h: through it the seven units of those see the context too) stands in a record each -- BedPipe .. MotifPipe.
#pragma once
#include "mc_dev.h"
#include "mc_own.h"

#include <atomic>
#include <string>

#ifndef MC_PASSES_IN_FLIGHT_N
#define MC_PASSES_IN_FLIGHT_N 6
#endif
// one being copied out, one in the side stream's kernels, one computing, two or three queued: a pass is 0.6-0.7 ms from its strand resolve
// to its records in host memory, and the ctx stream takes a new one every 0.21 ms (four in flight left it waiting for the host)
constexpr int MC_PASSES_IN_FLIGHT = MC_PASSES_IN_FLIGHT_N;
constexpr int MC_ROW_TEXT_BLOCKS = 6;    // pinned blocks the rows of text leave in (mc_rowtext.hip): a pass's stays taken until the host has written it
static_assert(MC_ROW_TEXT_BLOCKS <= 8, "a block's handle is ticket * 8 + index");

constexpr size_t COPY_BY_KERNEL_MAX = (size_t)4 << 20;      // larger transfers go to the DMA engines
constexpr size_t COPY_BY_KERNEL_MAX_STREAMING = (size_t)64 << 20;     // ... a pass's records while text is being streamed in: see mc_wait_records_begin

// What K0 writes and K1 reads, per pass in flight
struct K0Set {
    NbDesc *desc = nullptr;
    int64_t *nb_f0 = nullptr;
};

// Where a pass writes: the synchronous pass has one (mc_ctx::sync), every pipelined pass in flight its own (AsyncBuf::B)
struct PassBufs {
    K0Set K;                   // strand resolve output of the pass
    Counters *cnt = nullptr;   // its counters (device)
    DevRecords O;              // device records of the pass (the synchronous pass: the fast path's buffers)
    Payload *sorted = nullptr; // the pass's payloads in file order (k1_list -> k1_emit, k1_rare_dev)
    int64_t *rare = nullptr;   // records k1_emit leaves to k1_rare / k1_rare_dev
    unsigned long long pass_no = 0;   // what Counters.irregular_pass holds if the pass classified a block irregular (never 0)
};

// ---- the device parser's host-side structures (kernels, their argument structs and constants: mc_devparse.inc) ----
struct KpHead {                 // device-side result block of one parse (copied to the host as it is)
    long long n_newlines, n_lines, n_rows;
    int n_seg, n_unknown;
    long long first_host_line;  // first line that needs the host parser (LLONG_MAX: none)
    int overflow;               // bit 0: more lines than the scratch holds, 1: segments, 2: unknown-contig lines
    int pad;
};
// (struct KpSeg: mc_dev.h -- the row writer on the device reads the names where the parser found them)
struct KpUnknown { long long line; long long off; int len; int pad; };

struct KpScratch {              // line-indexed (kp_parse -> kp_place), shared by all slots: the parses are ordered on one stream
    long long *line_start = nullptr;
    int32_t *pos = nullptr, *idx = nullptr, *ev = nullptr, *mu = nullptr, *contig = nullptr;
    uint32_t *name_off = nullptr;
    uint16_t *name_len = nullptr;
    uint8_t *fl = nullptr, *status = nullptr;
    long long *tile_cnt = nullptr, *tile_off = nullptr;      // newline tiles, then row blocks
    int64_t cap_lines = 0, cap_tiles = 0;
    Pool allocs{"device parser scratch"};
};

struct KpContigs {              // the reference's contig names on the device: open addressing, FNV-1a
    uint32_t *hash = nullptr;   // table_size entries: hash | 0 = empty (a zero hash is stored as 1)
    int32_t *id = nullptr;
    uint32_t *name_off = nullptr;   // per contig id
    uint32_t *name_len = nullptr;
    char *chars = nullptr;
    int table_mask = 0, n = 0;
    Pool allocs{"contig names"};
    std::vector<std::string> names; // what the table was built from
};

// One resident table.  A ctx owns MC_TABLE_SLOTS of them so that a file can go through the GPU as a sequence of shards:
// one being uploaded, one being scanned, the others waiting for their records to be handed out.  All device memory of a
// slot is allocated once (mc_ctx_reserve_tables, or by the first table that needs more) -- an upload is DMA transfers, no kernel
// (the first pass over the table validates it while it scans), no hipMalloc / hipFree.
struct SmallLayout {       // byte offsets of a table's small arrays inside one block: the same on the pinned host stage and on the device
    size_t seg_begin, seg_read, seg_contig, nb_row_begin, nb_seg_begin, nb_read, nb_repeat, nb_vflags, tile_nb, qual, total;
};

struct TableSlot {
    DevTable T;                        // the table in the slot (pointers into the slot's allocations)
    int64_t cap_rows = 0, cap_segs = 0, cap_reads = 0;
    int32_t *pos = nullptr, *idx = nullptr;
    int2 *evmu = nullptr;
    uint8_t *flags = nullptr;
    uint8_t *nbits = nullptr;          // the model-N bit column (DevTable::nbits)
    Pinned nbits_h;                    // ... packed here for a caller that passes none (mc_table_view::model_n_bits == NULL)
    uint16_t *xrel = nullptr;          // the index-relation column (DevTable::xrel)
    Pinned xrel_h;                     // ... packed here for a caller that passes none (mc_table_view::idx_rel_bits == NULL)
    uint16_t *prel = nullptr;          // the position-relation column (DevTable::prel)
    int2 *unit_pp = nullptr;           // the unit summaries (DevTable::unit_pp)
    NbDesc *nb_tmpl = nullptr;
    unsigned char *small_dev = nullptr;   // the small arrays: device block ...
    Pinned stage;                         // ... and pinned host stage
    double *qual = nullptr;            // read qualities that travelled with the table (in small_dev), or nullptr
    int32_t n_qual = 0;
    Event ev_uploaded;                 // the H2D transfers of the slot's table are done
    Event ev_up_start, ev_val_start, ev_valid;   // ... begin; the small arrays are in place (ctx stream)
    int refs = 0;                      // passes in flight that scan this table (+1 while the device parser fills the slot)
    bool holds_table = false;          // S.T describes the columns in the slot (set by fill_slot; cleared when a parse begins to
                                       // overwrite them or is abandoned): what mc_ctx_select_table may make current again
    // What the passes enqueued so far leave behind for the next one (host-side notes; the work is ordered by the ctx stream):
    int passes = 0;                    // passes enqueued over this table.  The first completes the validation flags (k1_scan,
                                       // SCAN_VALIDATE_SUMMARY / SCAN_VALIDATE); later ones classify on the flags
    bool summarized = false;           // the table's maker has written unit_pp and prel (part of the table, like nbits and xrel:
                                       // mc_ctx_select_table(as_new) keeps it)
    // the device parser (mc_ctx_parse_begin .. _finish)
    char *text = nullptr;              // the shard's text on the device
    int64_t cap_text = 0;
    KpHead *kp_head = nullptr;         // device result block, segments, unknown-contig tokens ...
    KpSeg *kp_segs = nullptr;
    KpUnknown *kp_unknown = nullptr;
    Pinned kp_head_h, kp_segs_h, kp_unknown_h;   // ... and their pinned host copies
    Pinned kp_flags_h;                 // pinned host copy of the flag column
    int64_t kp_cap_flags = 0;
    int kp_cap_segs = 0;
    Event ev_parsed, ev_text_up;
    int kp_state = 0;                  // 0: idle, 1: parse enqueued, 2: results handed out (mc_ctx_parse_end)
    bool from_parser = false;          // the slot's table was made by the device parser: its text and segments (kp_segs_h, sorted) are the table's
    int64_t kp_flags_sent = 0;
    std::vector<int64_t> kp_seg_row, kp_seg_off, kp_unk_off;
    std::vector<int32_t> kp_seg_contig, kp_seg_len, kp_unk_len;
    std::vector<uint8_t> kp_seg_ns;
    Pool kp_allocs{"device parser slot"};
    long long tmpl_ref = -1;           // reference version the name-block templates were built for (-1: not built)
    Pool allocs{"table slot"};
};

// The classifier of the context: one of four kinds is set at a time (mc_ctx_set_mlp / _forest / _simple_classifier / _svm)
struct Classifier {
    enum Kind { NONE = -1, MLP = 0, FOREST = 1, SIMPLE = 2, SVM = 3 };
    DevMlp M;
    DevForest F;
    DevSimple Sc;                      // -c LR / -c NBC
    DevSvm Vs;                         // -c SVM
    Pool pool{"classifier"};
    Kind kind = NONE;
    int n_in = 0;                      // inputs of the one that is set (0: none)
    const uint8_t *sub_of_char = nullptr;   // its key table (device)
    void clear() {
        pool.clear();
        M = DevMlp(); F = DevForest(); Sc = DevSimple(); Vs = DevSvm();
        kind = NONE; n_in = 0; sub_of_char = nullptr;
    }
    void set(Kind k, int n, const uint8_t *soc) { kind = k; n_in = n; sub_of_char = soc; }     // (the last step of a setter: the upload went through)
};

// stage boundaries of a pipelined pass: dependencies between the streams, and the kernel times.  Events between kernels of this
// GPU first, then (from EV_DONE on) the ones the host waits for before it reads pinned memory
enum {
    EV_K0_START, EV_K0_END, EV_SCAN_START, EV_SCAN_END, EV_EMIT_END, EV_K2_START, EV_K2_END,
    EV_LIST_END,     // the pass's payloads are in file order (k1_list): what its emit, on the side stream, waits for
    EV_EMIT_START,   // ... and when that emit began (a timed pass: its own time, not the wait for the side stream's turn)
    EV_DONE, EV_COPIED, EV_TEXT, EV_N
};

// pipelined passes (mc_extract_features_async / mc_wait_records): record sets of their own, exported to pinned host memory.
// B: where the pass writes; everything else is what only a pipelined pass has
struct AsyncBuf {
    PassBufs B;
    DevRecords H;              // pinned host memory
    Pinned st;                 // where the host reads the pass's counters (st.dev: the same block as the GPU sees it)
    unsigned char *pack = nullptr;   // what is copied out, packed by k_pack: device staging ...
    Pinned pack_host;                // ... and pinned host
    unsigned long long *chunk_cnt = nullptr;               // k_pack_count -> k_pack
    int32_t *piece_cnt = nullptr;                          // the fused dense pass: records of every piece (k1_fused -> k2_mlp)
    int32_t *piece_kw = nullptr;                           // ... its calls | their wide slot means << 16 (k1_fused -> the side stream's kernel)
    int64_t piece_cap = 0;
    size_t pack_bytes = 0;                                 // bytes of pack / pack_host
    int32_t *h_lo32 = nullptr;                             // in pack_host: the slot means' 32-bit parts, the wide ones' high halves,
    uint32_t *h_hi32 = nullptr;                            // the mask byte of every call (mc_calls_view)
    unsigned char *h_wmask = nullptr;
    int64_t h_n_wide = 0;
    int32_t *h_close32 = nullptr;                          // in pack_host: 32-bit closing rows (tables below 2^31 - 1 rows), else H.close_row
    bool close32 = false;
    bool narrow = false;                                   // the side kernel was told to pack narrow records (narrow_layout) where the pass allows it
    const uint16_t *h_close_lo16 = nullptr, *h_pos_lo16 = nullptr, *h_info_lo16 = nullptr;      // in pack_host: a pass that took them (else H.site_pos ...)
    const uint8_t *h_info_next = nullptr;
    const int32_t *h_runs = nullptr;
    int64_t h_n_runs = 0;
    int64_t h_copy_out_bytes = 0;                          // what the pass sent over the link
    int64_t h_n_calls = 0;
    Event ev[EV_N];
    mc_params prm;
    int64_t cap = 0, n_nb = 0;
    int k = 0;
    bool used = false, copying = false, timed = true;
    bool one_kernel = false;   // the side stream ran as one kernel (k2_mlp<.., PACK>): its end is ev[EV_DONE]
    int want_text = 0;         // the rows as text, made on the device (mc_ctx_row_text was on when the pass was enqueued)
    int text_block = -1;       // ... the pinned block they are on their way to (mc_wait_records_begin), -1: none
    bool emit_aside = false;   // the pass's emit ran on the side stream (the eight-lane emit of a sparse reference)
    int fused_room = 0;        // > 0: the pass ran as ONE kernel (k1_fused) with this many record slots per piece -- holes in between
    int64_t slots = 0;         // ... record slots in all
    int slot = -1;             // table slot the pass scans
    const double *qual = nullptr;   // read qualities it was enqueued with
    int32_t n_qual = 0;
    Pool dev_allocs{"pass buffers"}, k0_allocs{"strand resolve output"};
};

// rows of text made on the device (mc_rowtext.hip; mc_ctx_row_text): scratch and one text buffer on the device -- the passes'
// row writers run one after the other on the side stream --, pinned blocks on the host
struct RowTextCtx {
    int on = 0;
    char lab_meth[8] = {}, lab_unmeth[8] = {};
    int lab_meth_len = 0, lab_unmeth_len = 0;
    RowTextScratch S = {};
    int64_t cap_rec = 0, cap_rows = 0, cap_wide = 0, cap_num = 0;
    Pool allocs{"row text scratch"}, out_allocs{"row text"};
    char *out = nullptr;
    size_t out_cap = 0;
    double bytes_per_row = 0.0;        // room per call row (raised when a pass's rows did not fit)
    bool room_forced = false;          // (tests, MCALLER_ROW_TEXT_ROOM: a pass gets the room the estimate says, not what the buffers hold)
    struct Block {
        Pinned text, st;                   // the rows; the writer's RowTextStatus
        size_t cap = 0;
        std::atomic<int> busy{0};          // 0: free; else the ticket of the pass whose rows it holds (what mc_row_text_release must name)
    } blocks[MC_ROW_TEXT_BLOCKS];
    int next_ticket = 0;
    long long n_text = 0, n_no_block = 0, n_host_needed = 0, n_too_small = 0, n_other = 0;     // passes, by what became of their rows (MCALLER_VERBOSE)
    // the pass handed out last
    int last_block = -1;
    int64_t last_bytes = 0, last_rows = 0;
};

// the two pinned blocks a file is read through on its way to the device, and the events behind the copies out of them (mc_textfeed.h)
struct TextStages {
    Pinned stage[2];
    size_t cap = 0;
    Event ev[2];
    void release() {
        for (Pinned &p : stage) p.reset();
        cap = 0;
    }
};

// ---- a record per file pipeline (mc_textfeed.h): the pinned blocks its results are handed out in, the figures of its last call
// and what else outlives a call.  release(): what mc_<pipeline>_release frees, behind a sync of the streams (release_pipeline) ----
struct BedPipe {                       // the summary of a .diffs file (bed/mc_bedsum.hip)
    Grown out;
    mc_bed_stats stats = {};
    void release() { out.reset(); }
};
struct TrainPipe {                     // the matrices of a --training_tsv file (train/mc_trainrows.hip): X, the contexts, the labels' bytes
    Grown X, ctx;
    std::string labels;
    mc_train_rows_stats stats = {};
    void release() {
        X.reset(); ctx.reset();
        std::string().swap(labels);
    }
};
struct MergePipe {                     // the text of the merge behind `-t N` (merge/mc_rowmerge.hip)
    Grown out;
    mc_rows_merge_stats stats = {};
    void release() { out.reset(); }
};
struct FastqPipe {                     // the read qualities of a FASTQ file (fastq/mc_fastqual.hip): keys, offsets and means
    Grown pool, off, mean;
    mc_fastq_quality_stats stats = {};
    void release() { pool.reset(); off.reset(); mean.reset(); }
};
struct EvalPipe {                      // the evaluation file of a .diffs file against labelled positions (eval/mc_evalcalls.hip)
    Grown out;
    mc_eval_stats stats = {};
    void release() { out.reset(); }
};
struct CmpPipe {                       // the rows of two --vo BED files compared per site (compare/mc_bedcompare.hip)
    Grown out;
    mc_cmp_stats stats = {};
    int64_t unaligned = 0;             // (a lifted comparison) bed1's lines without an image
    void release() { out.reset(); }
};
struct CurPipe {                       // the rows and the BED lines of a native sample compared with a control (compare/mc_curcompare.inc)
    Grown out, bed;
    mc_cur_stats stats = {};
    void release() { out.reset(); bed.reset(); }
};
struct CluPipe {                       // the rows and the BED lines of a sample's sites split in two by their currents (compare/mc_sitecluster.inc)
    Grown out, bed;
    mc_clu_stats stats = {};
    void release() { out.reset(); bed.reset(); }
};
struct PhasePipe {                     // the pair rows, the read rows and the BED lines of a sample's linked sites (compare/mc_readphase.inc)
    Grown out, reads, bed;
    mc_phase_stats stats = {};
    void release() { out.reset(); reads.reset(); bed.reset(); }
};
// The coordinate map of an XMFA alignment (compare/mc_xmfamap.inc): on the device from mc_xmfa_map until the next such call or
// mc_xmfa_map_release; map[g1] = ordinal << 33 | g2 << 1 | flip, ~0: unmapped.  The view's host copies are pinned, and plain
// Pinned blocks, not Grown ones: each call allocates them anew at exactly the view's size
struct XmfaPipe {
    Pool allocs{"alignment map"};
    unsigned long long *map = nullptr;
    int64_t n1 = 0, n2 = 0;
    Pinned g2, flip;
    mc_xmfa_stats stats = {};
    void drop_map() {
        allocs.clear();
        map = nullptr;
        n1 = n2 = 0;
    }
    void release() {
        drop_map();
        g2.reset(); flip.reset();
    }
};
struct MotifPipe {                     // the rows of the motif finder (motifs/mc_motifscan.hip)
    Grown out;
    mc_motif_stats stats = {};
    mc_motif_iupac_stats iupac_stats = {};
    // --iterative (motifs/mc_motifiter.inc): the left-over sites' two planes, '+' then '-', and where the contigs stand in them
    Grown left;
    int64_t left_words = 0;
    std::vector<int64_t> left_starts;
    mc_motif_iter_stats iter_stats = {};
    // the two files of the motif profile (motifs/mc_motifprofile.inc)
    Grown profile_out, profile_nn;
    mc_motif_profile_stats profile_stats = {};
    void release() {
        out.reset(); left.reset();
        left_words = 0;
    }
    void release_profile() { profile_out.reset(); profile_nn.reset(); }
};

// The members' order is the order of construction, and its reverse the order of destruction (mc_ctx_destroy: `delete c` behind a
// sync of every stream): the streams stand first and go last, behind every event, allocation and pinned block used on them.
struct mc_ctx {
    int device = 0;
    Stream stream;
    Stream up_stream;                  // H2D of tables
    Stream parse_stream;               // the device parser's kernels (the text of the next shard is on its way on up_stream meanwhile)
    Stream copy_stream;
    Stream copy_stream2;               // pipelined passes alternate between the two: no turnaround gap between transfers
    Stream side_stream;                // classifier and packing of the pipelined passes
    Stream site_stream;                // the reduction's own queue: a shard's records are reduced beside the passes in flight
    Event ev[6];
    DevTable T;                        // the current table: a copy of slots[cur].T
    TableSlot slots[MC_TABLE_SLOTS];
    int cur = -1;                      // slot of the current table
    int held = -1;                     // slot of the pass handed out last (its records may still be reduced: mc_site_counts)
    DevTable last_T;                   // ... and that table
    bool in_rerun = false;             // mc_wait_records is re-running a pass synchronously
    KpScratch kp;                      // the device parser's line-indexed scratch and contig table
    KpContigs kc;
    int64_t res_rows = 0, res_segs = 0, res_reads = 0;     // mc_ctx_reserve_tables
    long long ref_version = 0;
    int64_t scratch_nb = 0, scratch_tiles = 0;             // what the per-pass scratch below is sized for
    Pool scratch_allocs{"pass scratch"};
    Pool own{"context"};               // what lives as long as the context: the synchronous pass's counters, the reduction's status words
    double *qual_own = nullptr;        // mc_ctx_set_read_quality's buffer
    int32_t n_qual_own = 0;
    Pool qual_allocs{"read qualities"};
    DevRef R;
    Classifier clf;
    double *qual = nullptr;
    int32_t n_qual = 0;
    PassBufs sync;           // the synchronous pass (mc_extract_features)
    DevRecords O;            // records of the last call (view: the fast path's buffers, or the merged ones)
    DevRecords H;            // pinned host copy of the last call's records (mc_fetch_records_view) ...
    Pinned H_pin[6];         // ... its blocks: feats, site_pos, site_seg, close_row, info, prob
    int h_k = 0;
    Pool lit_allocs{"literal path"};
    int32_t *tile_local = nullptr;
    int64_t *tile_first = nullptr;
    int64_t *group_sum = nullptr;
    int32_t *tile_cnt = nullptr, *tile_half = nullptr;
    long long *tile_chunk = nullptr;
    Payload *payload = nullptr;
    long long payload_cap = 0;
    int n_cu = 256;
    int emit_wgs = 4;              // resident k1_emit workgroups per CU (occupancy query)
    int last_k = 0;
    int64_t last_n = 0;
    int64_t last_slots = 0;        // record slots the records handed out last occupy on the device (a fused dense pass: with holes in between)
    int last_fused_room = 0, last_rerun = 0;   // how the pass handed out last ran (mc_last_pass_info)
    int last_scan_mode = -1;       // the scan mode (SCAN_*) of the pass planned last (mc_ctx_last_scan_mode)
    size_t pack_min_bytes = 0;     // a pass's packed block: at least this (what a pass that did not fit said it needed, and a quarter)
    int fused_scale = 1;           // the fused dense pass (k1_fused): room per piece x this (doubled when a piece ran out of room)
    int64_t ref_total_len = 0;    // bases of the marked reference (record capacity guess)
    float times[5] = {0, 0, 0, 0, 0};
    Pool ref_allocs{"reference"}, rec_allocs{"records"};
    int64_t payload_tiles = 0;     // tiles the payload buffer was sized for
    int payload_chunk = 0;         // ... and the chunk size
    AsyncBuf ab[MC_PASSES_IN_FLIGHT];
    RowTextCtx rt;
    int ab_head = 0, ab_tail = 0, ab_count = 0;
    unsigned long long pass_counter = 0;   // pass numbers (never 0)
    int timing_every = 1;          // pipelined passes: the two timing events go with every n-th pass (mc_ctx_set_pass_timing)
    long long pass_seq = 0;
    int last_timed = 1;            // whether the pass handed out last carried them
    // per-site reduction (mc_site_*): counts on the device, RCCL communicator
    int32_t *site_cnt = nullptr;      // [2 * n_sites]: n_meth | n_total
    int64_t *site_first = nullptr;    // [n_sites]
    int64_t site_n = 0;
    Pool site_allocs{"site counts"};
    unsigned long long *site_status = nullptr;          // [4] device: pending, not-a-site, cross-contig (k_site_counts)
    Pinned site_status_host;                            // pinned copy the host reads (written by a kernel: no DMA)
    void *comm = nullptr;             // ncclComm_t
    int comm_world = 1;
    // The seven units that take whole text files through the GPU (mc_textfeed.h).  Their calls are synchronous and never run side
    // by side, so they share the file reader's two pinned blocks and the events that say a block's copy is done (the merge's
    // output leaves through them too): grown on demand, freed by every mc_*_release.  What a call hands out is its pipeline's own
    // (the records above) and stays valid until the next call of that pipeline or its release:
    TextStages text_stages;
    BedPipe bed;
    TrainPipe tr;
    MergePipe mg;
    FastqPipe fq;
    EvalPipe eval;
    CmpPipe cmp;
    CurPipe currents;
    CluPipe clusters;
    PhasePipe phase;
    XmfaPipe xmfa;
    MotifPipe motif;
    // the figures of the last random-forest fit (mc_forest_fit.hip, through mc_internal_forest_stats)
    mc_forest_fit_stats forest_stats = {};
};

// ---- what crosses the units ----
int mc_sync_pass_streams(mc_ctx *c);                                       // mc_stream.hip: every stream a pass, an upload or a parse runs on
int mc_ensure_scratch(mc_ctx *c, int64_t n_nb, int64_t n_tiles);           // mc_stream.hip
int mc_copy_by_kernel(void *dst, const void *src, size_t bytes, hipStream_t st);   // mc_tables.hip (k_copy_bytes: mc_devparse.inc)
int mc_enqueue_row_text(mc_ctx *c, AsyncBuf &b, int64_t n, int64_t m, int64_t n_wide);   // mc_rowtext_host.hip
