// mc_stream.hip -- libmcaller_hip.so, the host side of the device code (gfx950 / MI355X): THE PASSES -- synchronous, pipelined,
// copy-out, re-run -- and the per-site reduction over the records of the pass handed out last.  The rest of the host side: mc_ctx.h
// (the context), mc_context.hip (life cycle, classifier setters), mc_tables.hip (table slots, the device parser mc_devparse.inc, the
// reference), mc_rowtext_host.hip (rows of text), mc_comm.hip (RCCL).  C ABI: include/mcaller_hip.h.  The kernels of the passes live
// in mc_k0.hip, mc_scan.hip, mc_emit.hip, mc_fused.hip, mc_literal.hip, mc_classify.hip, mc_rowtext.hip (shared structures: mc_dev.h; the
// row-by-row walk of one window: mc_rows.h; the digits of a printed double: mc_rowtext.h); their map:
//
// The reference's hot path (extract_contexts.py:147-291 + :199) as HIP kernels over a columnar event
// table resident in HBM:
//
//   text         kp_count / kp_scan / kp_starts / kp_parse / kp_count_rows / kp_place   the eventalign TEXT of a streamed shard
//                                parsed on the device (mc_devparse.inc): line starts, tokens, numbers, name blocks and segments,
//                                the columns written straight into a table slot -- the model-N bit column (one bit per row:
//                                the row's model k-mer is NNNNNN), the index- and position-relation columns (two bits per
//                                row each) and the unit summaries (first / last position of every eight rows) with them, put
//                                together in kp_place
//   per table     k_unit_columns  a table that arrives as columns (mc_ctx_upload_table*): unit summaries and the
//                                position-relation column from the position column, on the upload stream behind its transfer
//                                (a device-parsed table has them from kp_place).  Nothing else runs at upload: the first
//                                pass over a table validates it while it scans
//                (nb_template     the pass-independent fields of the name-block descriptors: inside the first k0_first_site over a table)
//   per pass     k0_first_site   first site row of every name block under the "new read" strand rule (:161-174) -> strand of
//                                the block; classifies the block (regular / no sites / irregular) in the same workgroup.  On
//                                a table no pass has validated yet the classification rests on the block's first rows
//                                (direction of the event index, position 0) and the scan confirms it
//                k0_classify / k0_extend   tables with repeated read names; irregular runs widened
//                k1_scan         THE SCAN: one wave per tile of 2048 rows, nothing persistent.  First pass over a table: the
//                                unit summaries and the two relation columns (two bits per row each: its event index and
//                                its position against those of the row before it, position 0; all written by the table's
//                                maker; 1.5 B/row in all) go from HBM into registers and every row is validated from its
//                                bits (positions non-decreasing? event index strictly monotone? -- what makes a name block
//                                "regular"); units of eight rows that can hold a site row are
//                                found with one extract from the strand bitmask (two words per unit, straight from L2) and
//                                listed in LDS, fetch their rows' positions and flag bytes, and their rows are tested for
//                                "last row of a window"; every closed window leaves a 32-byte payload.  Later passes over the
//                                same table read the unit summaries alone (1 B/row).  These two instances take a tile that
//                                lies inside ONE name block in a single batch (scan_whole_tile: the whole tile's columns
//                                requested at entry, one descriptor, one trip for the mask words, one list, one decide
//                                loop); tiles with a block edge go chunk by chunk.  One-base motifs, where every unit
//                                passes, stream the positions and the model-N bits, and on a first pass the index relations
//                                with them (4.375 B/row), comparing the positions in registers.
//                k1_group_scan / k1_list   file order of the windows; payloads gathered into it
//                k1_emit         eight lanes per window: which of the rows before its last row belong to which slot, slot
//                                means in NumPy pairwise order (fp64) from the rows' (event, model) pairs -> one flush record
//                                (a pipelined pass: on the side stream, in front of the pass's classifier and packing)
//                k1_fused        a dense reference (a one-base motif), pipelined passes: scan, ordering and emit as one kernel,
//                                fixed room per 960-row piece (mc_fused.hip)
//                k2_mlp          batched 7-H-1 tanh/logistic forward: one lane per record, weights as scalar operands, a quarter
//                                of the hidden units per SIMD (flush records: hidden layer in fp32, fp64 where a printed digit
//                                could depend on it)
//                k2_mlp<.., PACK>   the side stream of a pipelined pass as ONE kernel: the windows the emit left to the
//                                row-by-row walk (its own records'), the MLP, the records packed for the copy-out
//                k1_rare_dev, k_pack_count / k_pack   the same in kernels of their own (other classifiers than the MLP)
//                k3_forest, k3_simple, k3_svm   random forest / LR / NBC / SVM predict_proba;  k_literal / k_merge  irregular reads, row by row
//                k_rt_count / k_rt_scan / k_rt_wide / k_rt_digits / k_rt_rows<false> / k_rt_scan_len / k_rt_rows<true> / k_rt_copy   the
//                                rows of a streamed shard as TEXT, written behind its packed records (mc_rowtext.hip; mc_ctx_row_text):
//                                the digits of every 64-bit slot mean one lane per number, the rows one lane per record -- counted,
//                                placed by a scan, written --, the text sent to a pinned block
//                k_site_counts   per-site reduction (+ ncclAllReduce)
//                k_copy_bytes    small transfers by the compute units (the DMA engines serialise behind queued text)
//
// Equivalence with the sequential machine on regular blocks (one contig, positions non-decreasing, event
// index monotone in the direction the first site row implies, no site at contig position 0, read name not
// seen before) is argued in DESIGN.md; every other block is classified irregular and handled by the
// literal per-run kernel (k_literal) so results never depend on a CPU path.
#include "mc_ctx.h"

static int ensure_pinned(mc_ctx *c, int64_t n, int k) {
    if (c->H.capacity >= n && c->h_k == k) return 0;
    c->H = DevRecords();
    const int64_t cap = std::max<int64_t>(n + n / 4, 1 << 16);
    const size_t bytes[6] = {(size_t)cap * k * 8, (size_t)cap * 4, (size_t)cap * 4, (size_t)cap * 8, (size_t)cap * 4, (size_t)cap * 8};
    for (int i = 0; i < 6; ++i)
        if (int rc = c->H_pin[i].alloc(bytes[i])) return rc;
    c->H.feats = c->H_pin[0].get<double>(); c->H.site_pos = c->H_pin[1].get<int32_t>(); c->H.site_seg = c->H_pin[2].get<int32_t>();
    c->H.close_row = c->H_pin[3].get<int64_t>(); c->H.info = c->H_pin[4].get<uint32_t>(); c->H.prob = c->H_pin[5].get<double>();
    c->H.capacity = cap;
    c->h_k = k;
    return 0;
}

// D2H of everything but the probabilities (they follow when the classifier is done)
static int copy_out_features(mc_ctx *c, int64_t n, int k, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(c->H.feats, c->O.feats, (size_t)n * k * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->H.site_pos, c->O.site_pos, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->H.site_seg, c->O.site_seg, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->H.close_row, c->O.close_row, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->H.info, c->O.info, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    return 0;
}

// the classifier of the context over n records (mc_classify.hip)
static void launch_classifier(mc_ctx *c, hipStream_t st, const double *feats, int k, const int32_t *site_seg, const int32_t *seg_read,
                              const double *qual, const uint32_t *info, const uint8_t *submodel_in, int64_t n, double *prob,
                              const unsigned long long *n_dev, const unsigned int *overflow, const int32_t *piece_cnt = nullptr,
                              int piece_room = 0, int64_t n_pieces = 0) {
    mc_launch_classifier(c->clf.M, c->clf.F, c->clf.Sc, c->clf.Vs, c->n_cu, st, feats, k, site_seg, seg_read, qual, info, submodel_in, n, prob, n_dev, overflow,
                         piece_cnt, piece_room, n_pieces);
}

// marked positions are dense (a one-base motif): the scan instance that lists every unit of a tile, bigger payload chunks
static bool dense_reference(const mc_ctx *c) {
    return c->ref_total_len > 0 && (double)c->R.n_sites * 64.0 > (double)c->ref_total_len;
}

// the scratch all passes share (ordered by the ctx stream): tile descriptors / counts / chunks, strand-resolve output of
// the synchronous pass
int mc_ensure_scratch(mc_ctx *c, int64_t n_nb, int64_t n_tiles) {
    if (c->sync.K.desc && n_nb <= c->scratch_nb && n_tiles <= c->scratch_tiles) return 0;
    if (int rc = mc_sync_pass_streams(c)) return rc;
    c->scratch_allocs.clear();
    const int64_t res_tiles = c->res_rows ? (c->res_rows + TILE - 1) / TILE : 0;
    // (with head room: the tables of a stream differ by a few name blocks, and growing again means waiting for everything in flight)
    const int64_t nb = std::max<int64_t>(std::max<int64_t>(n_nb + n_nb / 4 + 64, c->res_segs), c->scratch_nb);
    const int64_t nt = std::max<int64_t>(std::max<int64_t>(n_tiles + n_tiles / 8 + 16, res_tiles), c->scratch_tiles);
    Pool &P = c->scratch_allocs;
    if (P.get(&c->sync.K.desc, (size_t)nb + 1) || P.get(&c->sync.K.nb_f0, (size_t)nb + 1) ||
        P.get(&c->tile_chunk, ((size_t)nt + 1) * NCHUNK) || P.get(&c->tile_local, (size_t)nt + 1) ||
        P.get(&c->group_sum, (size_t)(nt / GROUP + 2)) || P.get(&c->tile_cnt, (size_t)nt + 1) || P.get(&c->tile_half, (size_t)nt + 1) ||
        P.get(&c->tile_first, (size_t)nt + 1))
        return -10;
    c->scratch_nb = nb;
    c->scratch_tiles = nt;
    return 0;
}

static int alloc_records(Pool &pool, DevRecords &D, int64_t cap, int k) {
    D.capacity = cap;
    if (pool.get(&D.feats, (size_t)cap * k) || pool.get(&D.site_pos, (size_t)cap) ||
        pool.get(&D.site_seg, (size_t)cap) || pool.get(&D.close_row, (size_t)cap) ||
        pool.get(&D.info, (size_t)cap) || pool.get(&D.prob, (size_t)cap) || pool.get(&D.wmask, (size_t)cap))
        return -10;
    return 0;
}

static int ensure_records(mc_ctx *c, int64_t cap, int k) {
    const int64_t need_tiles = std::max<int64_t>(c->T.n_tiles, c->scratch_tiles);
    const int chunk = dense_reference(c) ? 256 : 64;
    if (c->sync.O.capacity >= cap && c->last_k == k && c->payload_tiles >= need_tiles && c->payload_chunk >= chunk) { c->O = c->sync.O; return 0; }
    if (int rc = mc_sync_pass_streams(c)) return rc;
    c->rec_allocs.clear();
    if (alloc_records(c->rec_allocs, c->sync.O, cap, k)) return -10;
    c->payload_tiles = need_tiles;
    // (the scan hands out payload slots beyond a tile's own PT in chunks; every tile may leave most of its last chunk unused)
    c->payload_cap = cap + (need_tiles + 1) * (PT + chunk);
    c->payload_chunk = chunk;
    if (c->rec_allocs.get(&c->sync.sorted, (size_t)cap) || c->rec_allocs.get(&c->sync.rare, (size_t)cap) || c->rec_allocs.get(&c->payload, (size_t)c->payload_cap)) return -10;
    c->last_k = k;
    c->O = c->sync.O;
    return 0;
}

// Irregular name blocks: literal row-by-row machine on the GPU, then merge with the fast path's records.
static int run_literal_path(mc_ctx *c, const mc_params *prm, int64_t *n_io) {
    const DevTable &T = c->T;
    const int k = prm->k;
    const int n_groups = (T.n_nb + GROUP - 1) / GROUP;
    LitArgs LA;
    LA.T = T; LA.R = c->R; LA.desc = c->sync.K.desc; LA.nb_f0 = c->sync.K.nb_f0; LA.qual = c->qual; LA.qual_thresh = prm->qual_thresh;
    LA.k = k; LA.skip_thresh = prm->skip_thresh; LA.tail_contig = prm->tail_contig; LA.entry_read = prm->entry_read;
    LA.entry_first_idx = prm->entry_first_idx;
    int32_t *run_cnt, *run_rows, *cnt_local, *rows_local;
    int64_t *cnt_group, *rows_group;
    Pool &P = c->lit_allocs;
    if (P.get(&run_cnt, (size_t)T.n_nb + 1) || P.get(&run_rows, (size_t)T.n_nb + 1) ||
        P.get(&cnt_local, (size_t)T.n_nb + 1) || P.get(&rows_local, (size_t)T.n_nb + 1) ||
        P.get(&cnt_group, (size_t)n_groups + 1) || P.get(&rows_group, (size_t)n_groups + 1))
        return -10;
    LA.run_cnt = run_cnt; LA.run_rows = run_rows; LA.cnt_local = cnt_local; LA.cnt_group = cnt_group;
    LA.rows_local = rows_local; LA.rows_group = rows_group; LA.scratch = nullptr; LA.L = DevRecords(); LA.write = 0;
    const unsigned g = (unsigned)((T.n_nb + 63) / 64);
    mc_launch_literal(LA, g, c->stream);
    mc_launch_group_scan(run_cnt, (int64_t)T.n_nb, cnt_local, cnt_group, c->stream);
    mc_launch_group_scan(run_rows, (int64_t)T.n_nb, rows_local, rows_group, c->stream);
    std::vector<int64_t> hc((size_t)n_groups), hr((size_t)n_groups);
    HIP_TRY(hipMemcpyAsync(hc.data(), cnt_group, (size_t)n_groups * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hr.data(), rows_group, (size_t)n_groups * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    int64_t n_lit = 0, n_rows_lit = 0;
    for (int i = 0; i < n_groups; ++i) { n_lit += hc[(size_t)i]; n_rows_lit += hr[(size_t)i]; }
    if (n_lit == 0) return 0;
    DevRecords L, M;
    double *scratch;
    const int64_t n_fast = *n_io;
    if (alloc_records(P, L, n_lit, k) || alloc_records(P, M, n_fast + n_lit, k) ||
        P.get(&scratch, (size_t)std::max<int64_t>(n_rows_lit, 1) * MC_MAX_K))
        return -10;
    LA.scratch = scratch; LA.L = L; LA.write = 1;
    mc_launch_literal(LA, g, c->stream);
    mc_launch_merge(c->O, n_fast, L, n_lit, M, k, c->stream);
    HIP_TRY(hipGetLastError());
    c->O = M;
    *n_io = n_fast + n_lit;
    return 0;
}

// How a pass goes about its table: decided when it is enqueued, from what the passes before it have left (TableSlot.passes).
struct PassPlan {
    bool first;          // no pass has validated the table: classification on the blocks' first rows, the scan validates every row
    int scan_mode;       // SCAN_*
};
static PassPlan plan_pass(mc_ctx *c) {
    PassPlan P;
    P.first = true;
    P.scan_mode = c->last_scan_mode = SCAN_VALIDATE;
    if (c->cur < 0) return P;
    TableSlot &S = c->slots[c->cur];
    // (a one-base motif: every unit is listed, summaries would not help.  The summaries and the position relations are the
    // table maker's columns: nothing is launched for them here)
    const bool summaries = !dense_reference(c) && S.summarized;
    if (S.passes > 0) {
        P.first = false;
        P.scan_mode = summaries ? SCAN_SUMMARY : SCAN_STREAM;
    } else if (summaries) {
        P.scan_mode = SCAN_VALIDATE_SUMMARY;
    }
    S.passes += 1;
    c->last_scan_mode = P.scan_mode;
    return P;
}

// K0 (strand resolve) of one pass on the ctx stream: counters zeroed, first site rows, classification.
// pipelined: null for the synchronous pass, which also widens the irregular set (k0_extend) -- what its literal path needs; a
// pipelined pass with an irregular block is thrown away and re-run synchronously, so it never looks at the result.
static int enqueue_k0(mc_ctx *c, const mc_params *prm, const PassBufs &B, const PassPlan &plan, const AsyncBuf *pipelined) {
    const DevTable &T = c->T;
    const K0Set &K = B.K;
    hipStream_t st = c->stream;
    const int k = prm->k;
    const bool lookback = T.has_repeats || prm->entry_read >= 0;      // a block may see name == last_read (:161)
    // (the name-block templates: once per (table, reference), made by the first pass's k0_first_site itself)
    const bool make_tmpl = c->cur >= 0 && c->slots[c->cur].tmpl_ref != c->ref_version;
    if (c->cur >= 0) c->slots[c->cur].tmpl_ref = c->ref_version;
    mc_launch_first_site(T, c->R, c->qual, prm->qual_thresh, k, K.desc, K.nb_f0, B.cnt, lookback ? 0 : 1, prm->skip_thresh, B.pass_no,
                         plan.first ? 1 : 0, make_tmpl ? 1 : 0, st);
    if (lookback) mc_launch_classify(T, c->R, K.desc, K.nb_f0, prm->entry_read, k, prm->skip_thresh, B.cnt, B.pass_no, st);
    if (!pipelined) mc_launch_extend(T, K.desc, K.nb_f0, prm->entry_read, B.cnt, B.pass_no, st);
    return 0;
}

// K1 (scan, order, emit) of one pass into the record set B.O, on the ctx stream but for a pipelined pass's eight-lane emit.
// pipelined: null for the synchronous pass, whose ev[2] is recorded after the scan; else the pass's events, chunk counts, room
// per piece (fused_room > 0: the pass as one kernel) and per-piece counts.
static int enqueue_k1(mc_ctx *c, const mc_params *prm, const PassBufs &B, const PassPlan &plan, const AsyncBuf *pipelined, K1Args *out_args) {
    const DevTable &T = c->T;
    hipStream_t st = c->stream;
    const AsyncBuf *b = pipelined;
    const int fused_room = b ? b->fused_room : 0;
    hipEvent_t ev_emit_end = b ? b->ev[EV_EMIT_END].e : nullptr, ev_list_end = b ? b->ev[EV_LIST_END].e : nullptr;
    K1Args A;
    A.T = T; A.R = c->R; A.desc = B.K.desc; A.tile_chunk = c->tile_chunk; A.payload = c->payload;
    A.payload_cap = c->payload_cap; A.tile_cnt = c->tile_cnt; A.tile_half = c->tile_half;
    A.tile_local = c->tile_local; A.group_sum = c->group_sum; A.tile_first = c->tile_first; A.O = B.O; A.cnt = B.cnt; A.k = prm->k;
    A.skip_thresh = prm->skip_thresh; A.tail_contig = prm->tail_contig; A.rare_list = B.rare;
    A.pass_no = B.pass_no;
    A.piece_cnt = b ? b->piece_cnt : nullptr;
    A.piece_kw = (fused_room > 0 && fused_room < MC_SIDE_MAX_ROOM) ? b->piece_kw : nullptr;
    const bool dense = dense_reference(c);                 // (its emit: the run table, k1_emit_runs)
    // (k1_emit and the row-by-row kernel count the packing's chunks as they write the records; the run-table emit of a dense
    // reference does not: k_pack_count goes over its records)
    A.chunk_cnt = (b && !dense) ? b->chunk_cnt : nullptr;
    A.chunk_shift = dense ? 8 : 6;
    A.shard_shift = T.n_tiles >= 1024 ? 6 : 3;
    A.shard_mask = (1 << A.shard_shift) - 1;
    static_assert(NSHARD == 64, "shard_shift");
    hipEvent_t on_packet = MC_EVENTS_ON_KERNELS ? ev_emit_end : nullptr;
    if (fused_room > 0) {
        // a dense reference, a pipelined pass: scan, ordering and emit as ONE kernel with fixed room per piece (k1_fused,
        // mc_fused.hip); the pass's event rides on its dispatch packet
        mc_launch_fused(A, B.sorted, fused_room, plan.first, st, on_packet);
        if (!on_packet) HIP_TRY(hipEventRecord(ev_emit_end, st));
        *out_args = A;
        return 0;
    }
    mc_launch_scan(A, dense, plan.scan_mode, st);
    if (!b) HIP_TRY(hipEventRecord(c->ev[2], st));
    mc_launch_group_scan(c->tile_cnt, T.n_tiles, c->tile_local, c->group_sum, st);
    // (dense references: a workgroup per piece, the mean of every position once, see k1_emit_runs -- which takes the payloads where
    // the scan left them: no gather)
    // The eight-lane emit of a pipelined pass goes to the SIDE stream, in front of the pass's classifier and packing: it reads nothing but
    // the pass's own buffers (its sorted payloads, descriptors, records, counters) and the table, is bound by latency (three dependent
    // round trips: 39 us with a few thousand waves), and on the ctx stream the next pass's strand resolve and scan waited behind it
    const bool emit_aside = b && !dense;
    mc_launch_list(A, B.sorted, dense ? 0 : 1, st, (emit_aside && MC_EVENTS_ON_KERNELS) ? ev_list_end : nullptr);
    // (ev_emit_end rides on the emit's own dispatch packet: a hipEventRecord behind it is a barrier packet of its own and
    // costs the queue 5-9 us)
    const unsigned emit_grid = (unsigned)std::min<int64_t>((B.O.capacity * EG + 255) / 256, (int64_t)c->n_cu * c->emit_wgs);
    hipStream_t est = st;
    if (emit_aside) {
        if (!MC_EVENTS_ON_KERNELS) HIP_TRY(hipEventRecord(ev_list_end, st));
        HIP_TRY(hipStreamWaitEvent(c->side_stream, ev_list_end, 0));
        est = c->side_stream;
    }
    if (dense) mc_launch_emit_runs(A, B.sorted, st, on_packet);
    else mc_launch_emit(A, B.sorted, emit_grid, est, on_packet, (emit_aside && on_packet && b->timed) ? b->ev[EV_EMIT_START].e : nullptr);
    if (b && !on_packet) HIP_TRY(hipEventRecord(ev_emit_end, est));
    *out_args = A;
    return 0;
}

// the synchronous pass: everything on the ctx stream, ev[0..3] around the stages (mc_last_times_ms)
static int enqueue_fast_path(mc_ctx *c, const mc_params *prm, K1Args *out_args) {
    const PassPlan plan = plan_pass(c);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (int rc = enqueue_k0(c, prm, c->sync, plan, nullptr)) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (int rc = enqueue_k1(c, prm, c->sync, plan, nullptr, out_args)) return rc;
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    return 0;
}

// Record capacity to start with: a window closes about once per marked site a read covers -- rows x (sites per strand
// position) x ~0.52 positions per row -- with 50 % head room, and never less than one per 64 rows (GATC in a random
// genome: one per ~490 rows).  A pass that overflows it is repeated with what it actually needed.
static int64_t guess_capacity(const mc_ctx *c) {
    if (const char *e = getenv("MCALLER_RECORD_CAPACITY")) { if (atoll(e) > 0) return atoll(e); }   // (tests: force the overflow path)
    const double density = c->ref_total_len > 0 ? (double)c->R.n_sites / (2.0 * (double)c->ref_total_len) : 0.0;
    const int64_t rows = std::max<int64_t>(c->T.n_rows, c->res_rows);        // (reserved: every later table fits, no re-allocation)
    const int64_t by_sites = (int64_t)((double)rows * density * 0.52 * 1.5);
    return std::max<int64_t>(1 << 16, std::max<int64_t>(rows / 64, by_sites) + 4096);
}

// what every pass needs before it can be enqueued
static int check_pass(mc_ctx *c, const mc_params *prm) {
    const DevTable &T = c->T;
    const int k = prm->k;
    if (k < 1 || k > MC_MAX_K) {
        mc_set_error("num_variables %d not supported (1..%d)", k, MC_MAX_K);
        return -12;
    }
    if (!T.pos || !c->R.mf || !c->qual) {
        mc_set_error("mc_extract_features: table, reference and read qualities must be set first");
        return -12;
    }
    if (c->n_qual < T.n_reads) {
        mc_set_error("read quality table has %d entries, table names %d reads", c->n_qual, T.n_reads);
        return -12;
    }
    const int clf_in = c->clf.n_in;
    if (prm->score && clf_in != k + 1) {
        mc_set_error("classifier expects %d inputs but num_variables+1 = %d", clf_in, k + 1);
        return -12;
    }
    return 0;
}

extern "C" int mc_extract_features(mc_ctx *c, const mc_params *prm, int64_t *n_records) {
    HIP_TRY(hipSetDevice(c->device));
    *n_records = 0;
    const DevTable &T = c->T;
    const int k = prm->k;
    if (int rc = check_pass(c, prm)) return rc;
    c->last_n = 0;
    c->last_slots = 0;
    if (T.n_rows == 0 || T.n_nb == 0) return 0;
    if (c->ab_count) { if (int rc = mc_sync_pass_streams(c)) return rc; }   // pipelined passes share the scratch: let them finish
    if (int rc = mc_ensure_scratch(c, T.n_nb, T.n_tiles)) return rc;
    c->last_T = T;
    if (!c->in_rerun) c->held = c->cur;                                   // (a re-run inside mc_wait_records: held by the caller)

    c->lit_allocs.clear();
    int64_t cap = std::max<int64_t>(guess_capacity(c), c->sync.O.capacity);
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (int rc = ensure_records(c, cap, k)) return rc;
        K1Args A;
        c->sync.pass_no = ++c->pass_counter;
        if (int rc = enqueue_fast_path(c, prm, &A)) return rc;
        Counters h;
        HIP_TRY(hipMemcpyAsync(&h, c->sync.cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipGetLastError());
        int64_t n = (int64_t)h.n_records;
        if (h.overflow) {                   // the buffers were a guess; the exact need is known now (+ shard skew)
            cap = std::max<int64_t>(cap * 2, n + n / 4 + 4096);
            continue;
        }
        // the table's first pass, and a row contradicts what a block was classified on (its first rows): the validation flags
        // are complete now, the next attempt classifies on them
        if (h.violation) continue;
        if (h.n_rare) {
            mc_launch_rare(A, c->sync.sorted, c->sync.rare, (int64_t)h.n_rare, c->stream);
        }
        if (h.n_big && n > 0) mc_launch_bigfix(A, n, c->stream);
        const bool irregular = h.irregular_pass == c->sync.pass_no;
        if (irregular) {
            if (int rc = run_literal_path(c, prm, &n)) return rc;
        }
        // records -> pinned host memory; the slot means and indices travel while the classifier runs
        if (int rc = ensure_pinned(c, n, k)) return rc;
        const bool early = n > 0 && !h.n_big && !h.n_rare && !irregular;      // (nothing on the ctx stream still writes records)
        if (early) { if (int rc = copy_out_features(c, n, k, c->copy_stream)) return rc; }
        if (prm->score && n > 0)
            launch_classifier(c, c->stream, c->O.feats, k, c->O.site_seg, T.seg_read, c->qual, c->O.info, (const uint8_t *)nullptr, n,
                              c->O.prob, (const unsigned long long *)nullptr, (const unsigned int *)nullptr);
        HIP_TRY(hipEventRecord(c->ev[4], c->stream));
        if (n > 0) {
            if (!early) { if (int rc = copy_out_features(c, n, k, c->stream)) return rc; }
            HIP_TRY(hipMemcpyAsync(c->H.prob, c->O.prob, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipStreamSynchronize(c->copy_stream));
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&c->times[i], c->ev[i], c->ev[i + 1]));
        HIP_TRY(hipEventElapsedTime(&c->times[4], c->ev[0], c->ev[4]));
        c->last_n = n;
        c->last_slots = n;
        *n_records = n;
        return 0;
    }
    mc_set_error("record buffer overflow after 4 attempts");
    return -13;
}

extern "C" int mc_fetch_records(mc_ctx *c, const mc_calls_view *out) {
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = c->last_n;
    const int k = c->last_k;
    if (out->capacity < n) {
        mc_set_error("mc_fetch_records: capacity %lld < %lld records", (long long)out->capacity, (long long)n);
        return -12;
    }
    if (n == 0) return 0;
    memcpy(out->feats, c->H.feats, (size_t)n * k * 8);
    memcpy(out->site_pos, c->H.site_pos, (size_t)n * 4);
    memcpy(out->site_seg, c->H.site_seg, (size_t)n * 4);
    memcpy(out->close_row, c->H.close_row, (size_t)n * 8);
    memcpy(out->info, c->H.info, (size_t)n * 4);
    memcpy(out->prob, c->H.prob, (size_t)n * 8);
    return 0;
}

extern "C" int mc_fetch_records_view(mc_ctx *c, mc_calls_view *out) {
    out->capacity = c->last_n;
    out->feats = c->H.feats;
    out->site_pos = c->H.site_pos;
    out->site_seg = c->H.site_seg;
    out->close_row = c->H.close_row;
    out->info = c->H.info;
    out->prob = c->H.prob;
    out->call_row = nullptr;          // means and probabilities are stored for every record here
    out->n_call_rows = 0;
    out->close_row32 = nullptr;
    out->compacted = 0;
    out->feats_lo32 = nullptr; out->feats_hi32 = nullptr; out->feats_wide = nullptr; out->n_wide = 0;
    out->close_lo16 = nullptr; out->pos_lo16 = nullptr; out->info_lo16 = nullptr; out->info_next = nullptr;
    out->runs = nullptr; out->n_runs = 0;
    out->copy_out_bytes = 0;          // (a synchronous pass: six plain copies, nothing packed)
    return 0;
}

// ---- pipelined passes ----
// A pass computes on the ctx stream (K0, K1, K2, packing, back to back with the next pass) and is copied out on
// copy_stream when it is waited for.
// cap: record slots; pack_rec: records the packed block is sized for (a fused pass: the records expected, not every slot -- ten
// gigabytes of pinned memory less at 10^8 rows; a pass that needs more is repeated and the next block is bigger)
static int ensure_async_buf(mc_ctx *c, AsyncBuf &b, int64_t cap, int k, int64_t pack_rec = 0) {
    const DevTable &T = c->T;
    if (!b.ev[EV_DONE]) {
        // events between kernels of this GPU (timing, the side stream's wait for the emit) need no system-scope fence -- without
        // it a record costs the queue ~5 us instead of ~9; the two the host waits for before it reads pinned memory (ev_done,
        // ev_copied) keep the default
        for (int i = 0; i < EV_N; ++i)
            if (int rc = b.ev[i].create(i < EV_DONE ? hipEventDisableSystemFence : hipEventDefault)) return rc;
    }
    // the strand-resolve output (64 B per name block) and the record set are sized apart: tables that come in turn differ by a few
    // name blocks, and that must not cost a record set (for a one-base motif: gigabytes, pinned) -- with head room, so that it
    // happens once
    if (b.n_nb < T.n_nb) {
        if (b.used) HIP_TRY(hipEventSynchronize(b.ev[EV_DONE]));
        b.k0_allocs.clear();
        const int64_t nb = std::max<int64_t>(T.n_nb + T.n_nb / 4 + 64, c->scratch_nb);
        if (b.k0_allocs.get(&b.B.K.desc, (size_t)nb + 1) || b.k0_allocs.get(&b.B.K.nb_f0, (size_t)nb + 1)) return -10;
        b.n_nb = nb;
    }
    if (pack_rec <= 0 || pack_rec > cap) pack_rec = cap;
    const size_t pack_bytes = std::max((size_t)pack_rec * (24 + ((size_t)k + 1) * 8 + 1) + 128, c->pack_min_bytes);       // (every slot mean 64 bits wide at worst, a mask byte per call; narrow records, every record a run of its own: 23 bytes)
    if (b.cap >= cap && b.k == k && b.pack_bytes >= pack_bytes) return 0;
    if (b.used) HIP_TRY(hipEventSynchronize(b.ev[EV_DONE]));
    b.dev_allocs.clear();
    b.H = DevRecords();
    if (alloc_records(b.dev_allocs, b.B.O, cap, k)) return -10;
    if (b.dev_allocs.get(&b.B.cnt, 1)) return -10;
    // (the pass mark is only ever written by the kernels: whatever fresh device memory holds must not look like a pass number)
    HIP_TRY(hipMemsetAsync(b.B.cnt, 0, sizeof(Counters), c->stream));
    if (cap >= (int64_t)1 << 31) {
        mc_set_error("mc_extract_features_async: %lld flush records per pass (call rows are 32 bits wide); use mc_extract_features",
                     (long long)cap);
        return -12;
    }
    if (b.dev_allocs.get(&b.pack, pack_bytes) || b.dev_allocs.get(&b.chunk_cnt, (size_t)PACK_PAD * PACK_WGS)) return -10;
    if (b.dev_allocs.get(&b.B.sorted, (size_t)cap) || b.dev_allocs.get(&b.B.rare, (size_t)cap)) return -10;
    b.piece_cap = cap / 16 + 64;                               // (a piece has at least 48 slots: mc_fused_room)
    if (b.dev_allocs.get(&b.piece_cnt, (size_t)b.piece_cap) || b.dev_allocs.get(&b.piece_kw, (size_t)b.piece_cap)) return -10;
    if (b.pack_host.alloc(pack_bytes)) return -10;
    b.pack_bytes = pack_bytes;
    b.H.capacity = cap;
    if (!b.st.p) { if (b.st.alloc(sizeof(Counters))) return -10; }
    b.cap = cap;
    b.k = k;
    b.used = false;
    return 0;
}

// Classifier of a pass whose emit has been enqueued (ev_emit_end recorded), on the side stream.
// In front of it the windows the emit left to the row-by-row kernel (longer than 64 rows; usually none): the pass has its
// own sorted payloads and list, so this need not hold up the next pass's strand resolve on the ctx stream.
static int enqueue_k2(mc_ctx *c, AsyncBuf &b, const K1Args &A) {
    const DevTable &T = c->T;
    hipStream_t st = c->side_stream;
    HIP_TRY(hipStreamWaitEvent(st, b.ev[EV_EMIT_END], 0));
    mc_launch_rare_dev(A, b.B.sorted, b.B.rare, st);
    if (b.timed || !MC_EVENTS_ON_KERNELS) HIP_TRY(hipEventRecord(b.ev[EV_K2_START], st));
    if (b.prm.score)
        launch_classifier(c, st, b.B.O.feats, b.k, b.B.O.site_seg, T.seg_read, c->qual, b.B.O.info, (const uint8_t *)nullptr, b.cap, b.B.O.prob,
                          (const unsigned long long *)&b.B.cnt->n_records, (const unsigned int *)&b.B.cnt->overflow,
                          b.fused_room > 0 ? b.piece_cnt : nullptr, b.fused_room, b.fused_room > 0 ? b.slots / b.fused_room : 0);
    if (b.timed || !MC_EVENTS_ON_KERNELS) HIP_TRY(hipEventRecord(b.ev[EV_K2_END], st));
    return 0;
}

// The side stream of a pass as ONE kernel (k2_mlp<.., PACK>, mc_classify.hip): the windows left to the row-by-row walk, the MLP,
// the packing -- every workgroup for its own records.  -> 1: enqueued (ev_done rides on it); 0: not for this pass (enqueue_k2 +
// enqueue_pack: k1_rare_dev, the context's classifier, k_pack_count / k_pack)
static int enqueue_side(mc_ctx *c, AsyncBuf &b, const K1Args &A, bool *done) {
    const DevTable &T = c->T;
    hipStream_t st = c->side_stream;
    *done = false;
    const bool other = c->clf.kind != Classifier::MLP && c->clf.kind != Classifier::NONE;
    if (b.prm.score && c->clf.kind != Classifier::MLP) return 0;
    HIP_TRY(hipStreamWaitEvent(st, b.ev[EV_EMIT_END], 0));
    if (b.timed || !MC_EVENTS_ON_KERNELS) HIP_TRY(hipEventRecord(b.ev[EV_K2_START], st));
    // narrow records (narrow_layout) for what the side kernel packs record by record: not the pieces of a fused dense pass, not 64-bit
    // closing rows, not a pass whose rows the device writes as text (mc_rowtext.hip reads the wide columns on the device).
    // (MCALLER_NARROW_RECORDS=0: tests, profiles -- the wide columns; read per pass)
    const bool narrow_off = getenv("MCALLER_NARROW_RECORDS") && atoi(getenv("MCALLER_NARROW_RECORDS")) == 0;
    b.narrow = !narrow_off && b.fused_room == 0 && b.close32 && !b.want_text;
    if (!mc_launch_side(c->clf.M, other, c->n_cu, st, A, b.B.sorted, T.seg_read, c->qual, b.cap, b.prm.score ? 1 : 0, b.pack, b.pack_bytes, b.close32 ? 1 : 0, (Counters *)b.st.dev,
                        b.fused_room, b.fused_room > 0 ? b.slots / b.fused_room : 0, MC_EVENTS_ON_KERNELS ? b.ev[EV_DONE] : nullptr, b.narrow ? 1 : 0)) {
        b.narrow = false;
        return 0;           // (the wait and the event stay where they are: harmless in front of the three kernels)
    }
    if (!MC_EVENTS_ON_KERNELS) HIP_TRY(hipEventRecord(b.ev[EV_DONE], st));
    HIP_TRY(hipGetLastError());
    *done = true;
    return 0;
}

// Packing of a pass whose classifier has been enqueued (ev_k2_end recorded): what mc_wait_records_begin copies out.
// count: the chunk counts are not there yet (the emit counts them as it writes the records, except k1_emit_runs)
static int enqueue_pack(mc_ctx *c, AsyncBuf &b, bool count) {
    hipStream_t s2 = c->side_stream;
    const int holes = b.fused_room > 0 ? 1 : 0;
    if (count) mc_launch_pack_count(b.B.O, b.B.cnt, b.k, b.chunk_cnt, holes, s2);
    mc_launch_pack(b.B.O, b.B.cnt, b.chunk_cnt, b.pack, b.pack_bytes, b.k, b.close32 ? 1 : 0, (Counters *)b.st.dev, holes, count ? 1 : 0, s2, MC_EVENTS_ON_KERNELS ? b.ev[EV_DONE] : nullptr);
    if (!MC_EVENTS_ON_KERNELS) HIP_TRY(hipEventRecord(b.ev[EV_DONE], s2));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mc_extract_features_async(mc_ctx *c, const mc_params *prm) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = check_pass(c, prm)) return rc;
    if (c->ab_count >= MC_PASSES_IN_FLIGHT) {
        mc_set_error("mc_extract_features_async: %d passes are in flight; call mc_wait_records first", MC_PASSES_IN_FLIGHT);
        return -12;
    }
    const DevTable &T = c->T;
    const int k = prm->k;
    AsyncBuf &b = c->ab[c->ab_head];
    b.prm = *prm;
    if (T.n_rows == 0 || T.n_nb == 0) {            // nothing to scan: an empty pass
        if (int rc = ensure_async_buf(c, b, 1 << 16, k)) return rc;
        memset(b.st.p, 0, sizeof(Counters));
        b.B.pass_no = ++c->pass_counter;
        b.used = false;
        b.want_text = 0; b.text_block = -1;
        b.narrow = false;
        b.fused_room = 0; b.slots = 0;
        b.slot = -1;
        c->ab_head = (c->ab_head + 1) % MC_PASSES_IN_FLIGHT;
        c->ab_count += 1;
        return 0;
    }
    int64_t cap = std::max<int64_t>(guess_capacity(c), c->sync.O.capacity);
    // A dense reference (a one-base motif): the pass as ONE kernel with fixed room per piece of the table, holes in between
    // (k1_fused; MCALLER_DENSE_FUSED=0: the scan + emit pair, which the synchronous interface and every repeated pass keep)
    const bool fused_wanted = !(getenv("MCALLER_DENSE_FUSED") && atoi(getenv("MCALLER_DENSE_FUSED")) == 0);
    int fused_room = 0;
    if (fused_wanted && dense_reference(c)) {
        const double density = (double)c->R.n_sites / (2.0 * (double)c->ref_total_len);
        if (const char *e = getenv("MCALLER_FUSED_ROOM")) fused_room = std::max(1, atoi(e));        // (tests: force the overflow path)
        else fused_room = (int)std::min<int64_t>(mc_fused_room_max(), (int64_t)mc_fused_room(density) * c->fused_scale);
        cap = std::max<int64_t>(cap, mc_fused_pieces(T) * fused_room);
    }
    b.fused_room = fused_room;
    b.slots = fused_room > 0 ? mc_fused_pieces(T) * fused_room : 0;
    if (int rc = mc_ensure_scratch(c, T.n_nb, T.n_tiles)) return rc;
    if (int rc = ensure_records(c, cap, k)) return rc;          // the scratch all passes share (payloads, lists)
    int64_t pack_rec = fused_room > 0 ? std::min<int64_t>(cap, std::max<int64_t>(guess_capacity(c), c->sync.O.capacity)) : cap;
    if (const char *e = getenv("MCALLER_PACK_RECORDS")) { if (atoll(e) > 0) pack_rec = std::min<int64_t>(cap, atoll(e)); }      // (tests: a packed block that is too small)
    if (int rc = ensure_async_buf(c, b, cap, k, pack_rec)) return rc;
    if (fused_room > 0 && mc_fused_pieces(T) > b.piece_cap) { b.fused_room = 0; b.slots = 0; }     // (room forced very small: more pieces than counts)
    for (auto &other : c->ab)               // all record sets at once: no (pinned) allocation later, in the middle of a stream
        if (!other.used && (other.cap < cap || other.n_nb < T.n_nb || other.pack_bytes < b.pack_bytes)) { if (int rc = ensure_async_buf(c, other, cap, k, pack_rec)) return rc; }
    // K0 (strand resolve), the scan and the ordering of a pass on the ctx stream, back to back with the next pass: nothing on the
    // scan's path waits for another queue.  The eight-lane EMIT of a sparse reference, K2 (classifier) and the packing on the side
    // stream, behind the pass's ordering (an event on k1_list's dispatch packet): three dependent round trips with a few thousand
    // waves, 39 us during which the next pass's strand resolve and scan stood in the queue behind it -- beside the scan it takes 70-120
    // us and nobody waits for it.  The ctx stream takes a new pass every 0.21 ms then, and a pass is 0.6-0.7 ms from its strand
    // resolve to its records in host memory: with four passes in flight at most the ctx stream ran dry every second pass waiting for
    // the host (the emit on the side stream: 0.264 against 0.262 ms per pass); with six at most, four or five kept in flight: 0.242.
    // (The fused kernel of a dense reference and the run-table emit stay where they are: the one is the scan, the other reads the
    // scan's shared scratch.)
    // Measured earlier on the 10^8-row table (rocprofv3 timelines), passes per second relative to the layout with the emit on the ctx stream:
    // K0 on the side stream beside K2 on the ctx stream -3 % (two cross-queue hand-overs of 15-25 us on the scan's path);
    // K2 + packing deferred so that they run beside the next SCAN: the same (K2 gets one wave per SIMD there and takes 195 us
    // instead of 68); separate streams for K0 and K2: they land on one hardware queue and serialise; low-priority side
    // streams: time-sliced, 40 % slower; K0 of the next pass on a stream of its own, enqueued a whole pass ahead (it touches
    // nothing but the pass's own buffers): 0.286 ms per pass instead of 0.206 (a fifth stream shares a hardware queue), 0.238
    // with GPU_MAX_HW_QUEUES=8 -- which by itself costs 9 % (0.225); odd and even passes on two streams, the scan of a pass
    // waiting for the ordering kernels of the pass before it (the scratch they share) so that it runs beside that pass's emit,
    // one copy stream: 0.268 ms -- the kernels take what they take alone, the queues hand over slowly; the classifier in front
    // of k1_rare_dev (and once more behind it, if that kernel had a window to finish), so that it starts 8 us earlier and
    // runs less beside the scan: 0.2055 instead of 0.1985.
    hipStream_t st = c->stream;
    if (!c->side_stream) { if (int rc = c->side_stream.create()) return rc; }
    // (a hipEventRecord between two kernels costs this queue ~9 us -- rocprofv3 timeline -- so the two events that only time
    // the pass, unlike ev_emit_end, which the side stream waits for, can be thinned out: mc_ctx_set_pass_timing)
    b.timed = c->timing_every > 0 && (c->pass_seq++ % c->timing_every) == 0;
    const PassPlan plan = plan_pass(c);
    if (b.timed) HIP_TRY(hipEventRecord(b.ev[EV_K0_START], st));
    // (the buffer's last pass has been handed out, nothing on the device writes st_host: the mark mc_wait_records_begin looks for)
    b.st.get<Counters>()->side_done = ST_UNPUBLISHED;
    b.B.pass_no = ++c->pass_counter;
    if (int rc = enqueue_k0(c, prm, b.B, plan, &b)) return rc;
    if (b.timed) HIP_TRY(hipEventRecord(b.ev[EV_SCAN_START], st));
    K1Args A;
    // (no event between the scan and the ordering kernels here: a record costs the queue ~5 us; the feature extraction is timed
    // as one span, the split into scan and emit comes from mc_extract_features or from rocprofv3)
    if (int rc = enqueue_k1(c, prm, b.B, plan, &b, &A)) return rc;
    b.emit_aside = !dense_reference(c);         // (the eight-lane emit of a sparse reference: on the side stream)
    b.close32 = T.n_rows < INT32_MAX;           // (a closing row can be n_rows itself: the next shard's first row)
    b.want_text = c->rt.on;
    b.text_block = -1;
    b.one_kernel = false;
    b.narrow = false;
    if (int rc = enqueue_side(c, b, A, &b.one_kernel)) return rc;
    if (!b.one_kernel) {
        if (int rc = enqueue_k2(c, b, A)) return rc;
        if (int rc = enqueue_pack(c, b, A.chunk_cnt == nullptr)) return rc;
    }
    // (nothing goes on the copy stream here: it is a FIFO, and a wait for THIS pass queued now would hold back the
    // copy-out of the previous pass, which mc_wait_records enqueues later)
    HIP_TRY(hipGetLastError());
    b.used = true;
    b.slot = c->cur;
    b.qual = c->qual;
    b.n_qual = c->n_qual;
    if (b.slot >= 0) c->slots[b.slot].refs += 1;        // the table stays in its slot until the pass has been handed out
    c->ab_head = (c->ab_head + 1) % MC_PASSES_IN_FLIGHT;
    c->ab_count += 1;
    return 0;
}

int mc_sync_pass_streams(mc_ctx *c) {
    if (c->up_stream) HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    if (c->side_stream) HIP_TRY(hipStreamSynchronize(c->side_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream2));
    return 0;
}

// Copy-out of the oldest pass in flight whose copy-out has not been started, started but not waited for: the counters are
// read (k_pack left them in pinned memory; a wait for the pass's kernels), then one DMA transfer of exactly what the pass
// produced is enqueued on the copy stream.  Called for pass i+1 before mc_wait_records(i), the transfers run back to back:
// no host round trip sits between two copy-outs.  (No-op when every pass in flight is being copied out already.)
extern "C" int mc_wait_records_begin(mc_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->ab_count == 0) {
        mc_set_error("mc_wait_records_begin: no pass in flight");
        return -12;
    }
    int at = c->ab_tail, left = c->ab_count;
    while (left > 0 && c->ab[at].copying) { at = (at + 1) % MC_PASSES_IN_FLIGHT; --left; }
    if (left == 0) return 0;
    AsyncBuf &b = c->ab[at];
    // (two copy streams, taken in turn: a transfer that is enqueued while the previous one runs starts beside its tail; on
    // one stream 15-20 us pass between the end of one transfer and the start of the next -- rocprofv3 timeline -- which is
    // 8 % of a pass that the copy-out bounds)
    hipStream_t cs = (at & 1) ? c->copy_stream2 : c->copy_stream;
    if (b.used) {                                                // the counters (k_pack stored them in st_host), then exactly
        HIP_TRY(hipEventSynchronize(b.ev[EV_DONE]));                 // n records with the DMA engines
        HIP_TRY(hipStreamWaitEvent(cs, b.ev[EV_DONE], 0));
    }
    const Counters &st = *b.st.get<Counters>();
    unsigned char *pack_host = b.pack_host.get<unsigned char>();
    // (the pass's kernels are through: a block that still carries the mark of the enqueue was never written -- what it holds is an
    // earlier pass's, and no copy may be sized from it)
    if (b.used && st.side_done == ST_UNPUBLISHED) {
        mc_set_error("mc_wait_records_begin: pass %llu did not publish its counters", (unsigned long long)b.B.pass_no);
        return -12;
    }
    const bool special = st.overflow || st.irregular_pass == b.B.pass_no;      // (long windows were finished on the device: k1_rare_dev)
    if (b.used && !special && st.n_records > 0) {
        const size_t n = (size_t)std::min<int64_t>((int64_t)st.n_records, b.cap);
        const int k = b.k;
        const size_t m = (size_t)std::min<unsigned long long>(st.n_kept, n);
        const PackLayout L = pack_layout((int64_t)n, b.close32 ? 1 : 0);
        const size_t n_wide = (size_t)std::min<unsigned long long>(st.n_wide, (unsigned long long)m * (size_t)k);
        // (narrow records: the side kernel says whether the pass took them -- a run list of at least one entry -- or left the columns wide)
        const size_t n_runs = b.narrow ? (size_t)std::min<unsigned long long>(st.n_runs, (unsigned long long)n) : 0;
        const bool narrow = n_runs > 0;
        const NarrowLayout NL = narrow_layout((int64_t)n, (int64_t)n_runs);
        const PackTail PT_ = pack_tail(narrow ? NL.feats : L.feats, m, k, n_wide);
        const size_t out_bytes = PT_.end;
        if (out_bytes > b.pack_bytes) {
            mc_set_error("mc_wait_records_begin: pass %llu counts %zu bytes of records, its packed block holds %zu",
                         (unsigned long long)b.B.pass_no, out_bytes, b.pack_bytes);
            return -12;
        }
        // (a small record set -- a shard of a streamed file -- by kernel: the DMA engines may be busy with text, see k_copy_bytes;
        // and on the side stream, right behind the packing: the runtime folds the streams of a process onto four hardware
        // queues, and a copy stream that shares one with the parse stream would wait behind the kernels of the shards ahead,
        // which wait for their text)
        // (... and while shards of TEXT are on their way -- a slot is being parsed -- also a big one: the 7 MB of a dense shard's
        // records queued behind six shards of text, 2.5 ms each, and the host waited 0.24 s per 10^8 rows for records that were
        // long computed.  Resident tables, nothing on the link: the DMA engines, which do not go through the shader caches)
        static const size_t by_kernel_env = getenv("MCALLER_RECORDS_BY_KERNEL_MAX") ? (size_t)atoll(getenv("MCALLER_RECORDS_BY_KERNEL_MAX")) : 0;
        bool text_on_the_link = false;
        for (const TableSlot &S : c->slots) text_on_the_link = text_on_the_link || S.kp_state == 1;
        const size_t by_kernel_max = by_kernel_env ? by_kernel_env : (text_on_the_link ? COPY_BY_KERNEL_MAX_STREAMING : COPY_BY_KERNEL_MAX);
        if (out_bytes <= by_kernel_max && c->side_stream) {
            cs = c->side_stream;
            if (int rc = mc_copy_by_kernel(pack_host, b.pack, out_bytes, cs)) return rc;
        } else HIP_TRY(hipMemcpyAsync(pack_host, b.pack, out_bytes, hipMemcpyDeviceToHost, cs));
        b.H.close_row = (b.close32 || narrow) ? nullptr : reinterpret_cast<int64_t *>(pack_host);
        b.h_close32 = (b.close32 && !narrow) ? reinterpret_cast<int32_t *>(pack_host) : nullptr;
        b.H.site_pos = narrow ? nullptr : reinterpret_cast<int32_t *>(pack_host + L.pos);
        b.H.site_seg = narrow ? nullptr : reinterpret_cast<int32_t *>(pack_host + L.seg);
        b.H.info = narrow ? nullptr : reinterpret_cast<uint32_t *>(pack_host + L.info);
        b.h_close_lo16 = narrow ? reinterpret_cast<const uint16_t *>(pack_host + NL.close_lo) : nullptr;
        b.h_pos_lo16 = narrow ? reinterpret_cast<const uint16_t *>(pack_host + NL.pos_lo) : nullptr;
        b.h_info_lo16 = narrow ? reinterpret_cast<const uint16_t *>(pack_host + NL.info_lo) : nullptr;
        b.h_info_next = narrow ? pack_host + NL.info_next : nullptr;
        b.h_runs = narrow ? reinterpret_cast<const int32_t *>(pack_host + NL.runs) : nullptr;
        b.h_n_runs = (int64_t)n_runs;
        b.h_copy_out_bytes = (int64_t)out_bytes;
        b.H.feats = nullptr;                                             // (they travel as 32-bit integers where they can)
        b.h_lo32 = reinterpret_cast<int32_t *>(pack_host + PT_.lo32);
        b.H.prob = reinterpret_cast<double *>(pack_host + PT_.prob);
        b.h_wmask = pack_host + PT_.wmask;
        b.h_hi32 = reinterpret_cast<uint32_t *>(pack_host + PT_.hi32);
        b.h_n_wide = (int64_t)n_wide;
        b.h_n_calls = (int64_t)m;
        HIP_TRY(hipEventRecord(b.ev[EV_COPIED], cs));
        b.text_block = -1;
        if (b.want_text) { if (int rc = mc_enqueue_row_text(c, b, (int64_t)n, (int64_t)m, (int64_t)n_wide)) return rc; }
    }
    b.copying = true;
    return 0;
}

extern "C" int mc_wait_records(mc_ctx *c, int64_t *n_records, mc_calls_view *out) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->ab_count == 0) {
        mc_set_error("mc_wait_records: no pass in flight");
        return -12;
    }
    if (!c->ab[c->ab_tail].copying) { if (int rc = mc_wait_records_begin(c)) return rc; }
    AsyncBuf &b = c->ab[c->ab_tail];
    c->ab_tail = (c->ab_tail + 1) % MC_PASSES_IN_FLIGHT;
    c->ab_count -= 1;
    b.copying = false;
    // the pass leaves flight: its table stays put as "the table of the records handed out last" (mc_site_counts) until the
    // next pass is handed out
    if (b.slot >= 0) {
        c->slots[b.slot].refs -= 1;
        c->held = b.slot;
        c->last_T = c->slots[b.slot].T;
    }
    const Counters st = *b.st.get<Counters>();
    const bool special = st.overflow || st.irregular_pass == b.B.pass_no;
    if (b.used && !special && st.n_records > 0) HIP_TRY(hipEventSynchronize(b.ev[EV_COPIED]));
    c->rt.last_block = -1; c->rt.last_bytes = c->rt.last_rows = 0;
    if (b.text_block >= 0) {                                  // the rows as text (enqueue_row_text)
        auto &blk = c->rt.blocks[b.text_block];
        HIP_TRY(hipEventSynchronize(b.ev[EV_TEXT]));
        const RowTextStatus ts = *blk.st.get<RowTextStatus>();
        if (ts.too_small && st.n_kept > 0)
            c->rt.bytes_per_row = std::max(c->rt.bytes_per_row, 1.25 * (double)ts.n_bytes / (double)st.n_kept + 8.0);
        c->rt.n_host_needed += ts.host_needed ? 1 : 0;
        if (ts.host_needed && getenv("MCALLER_VERBOSE")) fprintf(stderr, "mcaller_hip: a pass's rows left to the host formatter (reasons 0x%x)\n", ts.host_needed);
        c->rt.n_too_small += ts.too_small ? 1 : 0;
        if (special || ts.host_needed || ts.too_small || ts.n_bytes > blk.cap) blk.busy.store(0);
        else { c->rt.n_text += 1; c->rt.last_block = b.text_block; c->rt.last_bytes = (int64_t)ts.n_bytes; c->rt.last_rows = (int64_t)ts.n_rows; }
        b.text_block = -1;
    }
    if (special && getenv("MCALLER_VERBOSE"))
        fprintf(stderr, "mcaller_hip: pass re-run synchronously (overflow %u, irregular %u, big %u, rare %u, records %llu)\n",
                st.overflow, (unsigned)(st.irregular_pass == b.B.pass_no), st.n_big, st.n_rare, st.n_records);
    c->last_fused_room = b.used ? b.fused_room : 0;
    c->last_rerun = special ? 1 : 0;
    if (special && st.overflow && st.pack_need > 0)           // (the packed block was too small: the next one holds that and a quarter)
        c->pack_min_bytes = std::max(c->pack_min_bytes, (size_t)st.pack_need + (size_t)st.pack_need / 4);
    else if (special && st.overflow && b.fused_room > 0 && b.fused_room < mc_fused_room_max())
        c->fused_scale = std::min(c->fused_scale * 2, 64);       // (a piece ran out of room: twice the room from the next pass on)
    if (special) {
        // a pass the fast path alone cannot finish (record buffers too small, irregular reads):
        // run it again through mc_extract_features, which handles all of that, and hand out its buffers
        // (on the table the pass was enqueued for, which need not be the current one any more)
        int64_t n = 0;
        const DevTable T_now = c->T;
        const double *q_now = c->qual;
        const int cur_now = c->cur, nq_now = c->n_qual;
        if (b.slot >= 0) { c->T = c->slots[b.slot].T; c->qual = const_cast<double *>(b.qual); c->n_qual = b.n_qual; c->cur = b.slot; }
        c->in_rerun = true;
        const int rc = mc_extract_features(c, &b.prm, &n);
        c->in_rerun = false;
        c->T = T_now; c->qual = const_cast<double *>(q_now); c->n_qual = nq_now; c->cur = cur_now;
        if (rc) return rc;
        c->last_timed = 1;         // (mc_extract_features times every pass)
        *n_records = n;
        return mc_fetch_records_view(c, out);
    }
    const int64_t n = (int64_t)st.n_records;
    c->last_timed = (b.used && b.timed) ? 1 : 0;
    if (b.used && b.timed) {
        float t_k0 = 0, t_scan = 0, t_emit = 0, t_k2 = 0;
        HIP_TRY(hipEventElapsedTime(&t_k0, b.ev[EV_K0_START], b.ev[EV_SCAN_START]));
        if (b.emit_aside && MC_EVENTS_ON_KERNELS) {
            // (the emit ran on the side stream: the ctx stream's span ends with the ordering, the emit's own time beside it)
            HIP_TRY(hipEventElapsedTime(&t_scan, b.ev[EV_SCAN_START], b.ev[EV_LIST_END]));
            HIP_TRY(hipEventElapsedTime(&t_emit, b.ev[EV_EMIT_START], b.ev[EV_EMIT_END]));
        } else {
            HIP_TRY(hipEventElapsedTime(&t_scan, b.ev[EV_SCAN_START], b.ev[EV_EMIT_END]));     // scan + ordering + emit, one span
            t_emit = 0.0f;
        }
        HIP_TRY(hipEventElapsedTime(&t_k2, b.ev[EV_K2_START], b.one_kernel ? b.ev[EV_DONE] : b.ev[EV_K2_END]));
        c->times[0] = t_k0; c->times[1] = t_scan; c->times[2] = t_emit; c->times[3] = t_k2;
        c->times[4] = t_k0 + t_scan + t_emit + t_k2;
    }
    c->O = b.B.O;                    // what mc_site_counts reduces: the records of the pass just handed out
    c->last_n = n;
    c->last_slots = b.fused_room > 0 ? std::min<int64_t>(b.slots, b.cap) : n;
    c->last_k = b.k ? b.k : c->last_k;
    *n_records = n;
    out->capacity = n;
    out->feats = b.H.feats; out->site_pos = b.H.site_pos; out->site_seg = b.H.site_seg;
    out->close_row = b.H.close_row; out->info = b.H.info; out->prob = b.H.prob;
    out->close_row32 = b.h_close32;
    out->call_row = nullptr;       // (not sent: the row of record j is the number of records before it without MC_I_TOO_MANY)
    out->compacted = 1;
    const bool packed = n > 0 && b.used;
    out->feats_lo32 = packed ? b.h_lo32 : nullptr;
    out->feats_hi32 = packed ? b.h_hi32 : nullptr;
    out->feats_wide = packed ? b.h_wmask : nullptr;
    out->n_wide = packed ? b.h_n_wide : 0;
    out->n_call_rows = n > 0 && b.used ? b.h_n_calls : 0;
    const bool narrow = packed && b.h_n_runs > 0;
    out->close_lo16 = narrow ? b.h_close_lo16 : nullptr;
    out->pos_lo16 = narrow ? b.h_pos_lo16 : nullptr;
    out->info_lo16 = narrow ? b.h_info_lo16 : nullptr;
    out->info_next = narrow ? b.h_info_next : nullptr;
    out->runs = narrow ? b.h_runs : nullptr;
    out->n_runs = narrow ? b.h_n_runs : 0;
    out->copy_out_bytes = packed ? b.h_copy_out_bytes : 0;
    return 0;
}

extern "C" int mc_last_pass_info(mc_ctx *c, int32_t *fused_room, int32_t *rerun) {
    if (fused_room) *fused_room = c->last_fused_room;
    if (rerun) *rerun = c->last_rerun;
    return 0;
}

extern "C" int mc_ctx_last_scan_mode(mc_ctx *c) { return c->last_scan_mode; }

// (tests) the scan's whole-tile predicate, evaluated on the host over the descriptors the synchronous pass left
extern "C" int64_t mc_ctx_whole_tiles(mc_ctx *c, uint8_t *per_tile) {
    HIP_TRY(hipSetDevice(c->device));
    const DevTable &T = c->T;
    if (c->cur < 0 || !c->sync.K.desc || T.n_nb <= 0 || T.n_nb > c->scratch_nb || T.n_tiles <= 0) {
        mc_set_error("mc_ctx_whole_tiles: no table, or no synchronous pass over it yet");
        return -12;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<NbDesc> desc((size_t)T.n_nb);
    std::vector<int32_t> tile_nb((size_t)T.n_tiles);
    HIP_TRY(hipMemcpy(desc.data(), c->sync.K.desc, desc.size() * sizeof(NbDesc), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tile_nb.data(), T.tile_nb, tile_nb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int64_t tile = 0; tile < T.n_tiles; ++tile) {
        const int64_t t0 = tile * TILE;
        int nb = tile_nb[(size_t)tile];                 // (as k1_scan finds the block of the tile's first row)
        if (nb < 0 || nb >= T.n_nb) { mc_set_error("mc_ctx_whole_tiles: tile %lld begins in block %d", (long long)tile, nb); return -12; }
        while (nb + 1 < T.n_nb && desc[(size_t)nb].row_end <= t0) ++nb;
        const bool whole = scan_tile_is_whole(desc[(size_t)nb], t0, (int)(std::min<int64_t>(t0 + TILE, T.n_rows) - t0));
        if (per_tile) per_tile[tile] = whole ? 1 : 0;
        n += whole;
    }
    return n;
}

extern "C" int mc_ctx_set_pass_timing(mc_ctx *c, int every_n) {
    if (every_n < 0) { mc_set_error("mc_ctx_set_pass_timing: every_n < 0"); return -12; }
    c->timing_every = every_n;
    return 0;
}

extern "C" int mc_last_pass_timed(mc_ctx *c) { return c->last_timed; }

extern "C" int mc_last_times_ms(mc_ctx *c, float *out5) {
    for (int i = 0; i < 5; ++i) out5[i] = c->times[i];
    return 0;
}

// predict_proba of the context's classifier on n input rows from the host (what the reference's call site :199 does, batched)
static int classifier_forward(mc_ctx *c, int which, const double *X, const uint8_t *submodel, int64_t n, double *p) {
    HIP_TRY(hipSetDevice(c->device));
    if (which != c->clf.kind) {                              // (which: a Classifier::Kind)
        mc_set_error("classifier forward: no %s set", which == 1 ? "forest" : (which == 2 ? "logistic / naive Bayes model" : (which == 3 ? "SVM" : "MLP")));
        return -12;
    }
    if (n <= 0) return 0;
    double *dX = nullptr, *dp = nullptr;
    uint8_t *ds = nullptr;
    const int ni = c->clf.n_in;
    Pool pool("classifier forward");
    if (pool.get(&dX, (size_t)n * ni) || pool.get(&dp, (size_t)n) || pool.get(&ds, (size_t)n)) return -10;
    HIP_TRY(hipMemcpyAsync(dX, X, (size_t)n * ni * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(ds, submodel, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dp, 0xFF, (size_t)n * 8, c->stream));   // NaN
    launch_classifier(c, c->stream, dX, ni - 1, (const int32_t *)nullptr, (const int32_t *)nullptr, (const double *)nullptr,
                      (const uint32_t *)nullptr, ds, n, dp, (const unsigned long long *)nullptr, (const unsigned int *)nullptr);
    HIP_TRY(hipMemcpyAsync(p, dp, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mc_mlp_forward(mc_ctx *c, const double *X, const uint8_t *submodel, int64_t n, double *p) {
    return classifier_forward(c, 0, X, submodel, n, p);
}

extern "C" int mc_forest_forward(mc_ctx *c, const double *X, const uint8_t *submodel, int64_t n, double *p) {
    return classifier_forward(c, 1, X, submodel, n, p);
}

extern "C" int mc_simple_forward(mc_ctx *c, const double *X, const uint8_t *submodel, int64_t n, double *p) {
    return classifier_forward(c, 2, X, submodel, n, p);
}

extern "C" int mc_svm_forward(mc_ctx *c, const double *X, const uint8_t *submodel, int64_t n, double *p) {
    return classifier_forward(c, 3, X, submodel, n, p);
}

// ===================================================================================================
// Per-site reduction feeding make_bed (make_bed.py:86-96: per (chrom, pos, strand) the list of 0/1 labels; :143,:154
// its mean and length; :134 rows in first-occurrence order).  Each rank counts its own records on the device; the
// one exchange step of the multi-GPU job is an all-reduce (sum of the counts, min of the first-seen row) over RCCL.
// ===================================================================================================
namespace {

// site number of (contig, strand, position); -1 if the position is not a marked site
__device__ __forceinline__ int64_t site_number(const DevRef &R, int contig, int rev, int64_t pos) {
    if (contig < 0 || contig >= R.n_contigs || pos < 0 || pos >= R.contig_len[contig]) return -1;
    const int64_t w = R.word_off[contig] + (pos >> 5);
    const uint32_t word = (rev ? R.mr : R.mf)[w];
    if (!((word >> (pos & 31)) & 1u)) return -1;
    const int before = (rev ? R.rank_r : R.rank_f)[w] + __popc(word & ((1u << (pos & 31)) - 1u));
    return R.site_base[contig * 2 + rev] + before;
}

__global__ void k_site_fill(int32_t *cnt, int64_t *first, int64_t n_sites) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < 2 * n_sites) cnt[i] = 0;
    if (i < n_sites) first[i] = INT64_MAX;
}

// one thread per flush record: scored, unskipped records add to their site (label 'm...' <=> p >= 0.5, :200).  make_bed
// keys a row on its chrom column, and that is the contig of the row that CLOSED the window (R8, :216): a record closed by a
// row of another contig is no site of the numbering -- counted in status[2] and left to the caller (a handful per file: the
// last window before a contig switch).
__global__ void k_site_counts(DevRef R, DevRecords O, int64_t n, DevTable T, int tail_contig, int64_t row_offset,
                              int32_t *__restrict__ cnt, int64_t *__restrict__ first, int64_t n_sites,
                              unsigned long long *__restrict__ status) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t info = O.info[j];
    if (info & MC_I_TOO_MANY) return;
    const int site_contig = T.seg_contig[O.site_seg[j]];
    const int64_t cr = O.close_row[j];
    int close_contig = tail_contig;
    if (cr < T.n_rows) {
        int lo = 0, hi = T.n_seg - 1;                               // last segment that begins at or before the closing row
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (T.seg_begin[mid] <= cr) lo = mid; else hi = mid - 1;
        }
        close_contig = T.seg_contig[lo];
    }
    if (close_contig != site_contig) { atomicAdd(&status[2], 1ull); return; }
    const double p = O.prob[j];
    if (p != p) { atomicAdd(&status[0], 1ull); return; }           // scored by the host (edge records): added by the caller
    const int64_t s = site_number(R, site_contig, (info & MC_I_REV) ? 1 : 0, O.site_pos[j]);
    if (s < 0) { atomicAdd(&status[1], 1ull); return; }
    atomicAdd(&cnt[n_sites + s], 1);
    if (p >= 0.5) atomicAdd(&cnt[s], 1);
    atomicMin(reinterpret_cast<long long *>(&first[s]), (long long)(O.close_row[j] + row_offset));
}

// the status words of one accumulation to where the host reads them; zeroed for the next
__global__ void k_site_status_out(unsigned long long *__restrict__ status, unsigned long long *__restrict__ host) {
    if (threadIdx.x < 4) {
        host[threadIdx.x] = status[threadIdx.x];
        status[threadIdx.x] = 0;
    }
}

}  // namespace

// The reduction has a queue of its own (site_stream): the records it reads are those of the pass handed out last -- complete
// since mc_wait_records returned --, so nothing of it has to wait for, or hold up, the passes in flight on the ctx stream
// (a shard's reduction used to drain that stream, allocate and free a status block, and fetch 24 bytes through the DMA
// engines, behind every shard of text on its way: 2 ms per shard).  What the host reads comes back through pinned memory
// written by a kernel.
static int ensure_site_buffers(mc_ctx *c) {
    const int64_t n = c->R.n_sites;
    if (!c->site_stream) { if (int rc = c->site_stream.create()) return rc; }
    if (!c->site_status) {
        if (c->own.get(&c->site_status, 32)) return -10;
        HIP_TRY(hipMemset(c->site_status, 0, 256));
    }
    if (!c->site_status_host.p) { if (c->site_status_host.alloc(256)) return -10; }
    if (c->site_cnt && c->site_n == n) return 0;
    HIP_TRY(hipStreamSynchronize(c->site_stream));
    c->site_allocs.clear();
    c->site_cnt = nullptr; c->site_first = nullptr;
    if (c->site_allocs.get(&c->site_cnt, (size_t)n * 2) || c->site_allocs.get(&c->site_first, (size_t)n)) return -10;
    c->site_n = n;
    return 0;
}

extern "C" int64_t mc_site_count(mc_ctx *c) { return c->R.n_sites; }

extern "C" int mc_site_counts_reset(mc_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->R.mf) {
        mc_set_error("mc_site_counts_reset: no reference set");
        return -12;
    }
    if (int rc = ensure_site_buffers(c)) return rc;
    const int64_t ns = c->R.n_sites;
    hipLaunchKernelGGL(k_site_fill, dim3((unsigned)((2 * ns + 255) / 256 + 1)), dim3(256), 0, c->site_stream, c->site_cnt, c->site_first, ns);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mc_site_counts(mc_ctx *c, int64_t row_offset, int32_t tail_contig, int64_t *n_pending, int64_t *n_cross_contig) {
    if (int rc = mc_site_counts_reset(c)) return rc;
    return mc_site_counts_accumulate(c, row_offset, tail_contig, n_pending, n_cross_contig);
}

extern "C" int mc_site_counts_accumulate(mc_ctx *c, int64_t row_offset, int32_t tail_contig, int64_t *n_pending, int64_t *n_cross_contig) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->R.mf || !c->site_cnt || c->site_n != c->R.n_sites) {
        mc_set_error("mc_site_counts_accumulate: call mc_site_counts_reset first (after the reference has been set)");
        return -12;
    }
    const int64_t ns = c->R.n_sites, n = c->last_slots;      // (every slot: a hole is a record that is not a call)
    if (n > 0)
        hipLaunchKernelGGL(k_site_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->site_stream, c->R, c->O, n,
                           c->last_T.seg_contig ? c->last_T : c->T, (int)tail_contig, row_offset, c->site_cnt,
                           c->site_first, ns, c->site_status);
    hipLaunchKernelGGL(k_site_status_out, dim3(1), dim3(64), 0, c->site_stream, c->site_status, (unsigned long long *)c->site_status_host.dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->site_stream));       // (this queue only: the passes in flight go on)
    const unsigned long long *sh = c->site_status_host.get<unsigned long long>();
    const unsigned long long h[3] = {sh[0], sh[1], sh[2]};
    if (h[1]) {
        mc_set_error("mc_site_counts: %llu records name a position that is not a marked site", h[1]);
        return -14;
    }
    if (n_pending) *n_pending = (int64_t)h[0];
    if (n_cross_contig) *n_cross_contig = (int64_t)h[2];
    return 0;
}

extern "C" int mc_site_counts_add(mc_ctx *c, const int64_t *site, const uint8_t *is_meth, const int64_t *first_row, int64_t n) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->site_cnt) {
        mc_set_error("mc_site_counts_add: call mc_site_counts first");
        return -12;
    }
    const int64_t ns = c->site_n;
    if (n <= 0) return 0;
    // rare (records the host scored itself): read-modify-write from the host
    std::vector<int32_t> cnt((size_t)ns * 2);
    std::vector<int64_t> first((size_t)ns);
    HIP_TRY(hipMemcpy(cnt.data(), c->site_cnt, (size_t)ns * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(first.data(), c->site_first, (size_t)ns * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
        const int64_t s = site[i];
        if (s < 0 || s >= ns) {
            mc_set_error("mc_site_counts_add: site %lld out of range", (long long)s);
            return -12;
        }
        cnt[(size_t)(ns + s)] += 1;
        if (is_meth[i]) cnt[(size_t)s] += 1;
        first[(size_t)s] = std::min(first[(size_t)s], first_row[i]);
    }
    HIP_TRY(hipMemcpy(c->site_cnt, cnt.data(), (size_t)ns * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->site_first, first.data(), (size_t)ns * 8, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int mc_site_counts_fetch(mc_ctx *c, int32_t *n_meth, int32_t *n_total, int64_t *first_row) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->site_cnt) {
        mc_set_error("mc_site_counts_fetch: call mc_site_counts first");
        return -12;
    }
    const int64_t ns = c->site_n;
    if (ns > 0) {
        HIP_TRY(hipMemcpyAsync(n_meth, c->site_cnt, (size_t)ns * 4, hipMemcpyDeviceToHost, c->site_stream));
        HIP_TRY(hipMemcpyAsync(n_total, c->site_cnt + ns, (size_t)ns * 4, hipMemcpyDeviceToHost, c->site_stream));
        HIP_TRY(hipMemcpyAsync(first_row, c->site_first, (size_t)ns * 8, hipMemcpyDeviceToHost, c->site_stream));
    }
    HIP_TRY(hipStreamSynchronize(c->site_stream));
    return 0;
}
