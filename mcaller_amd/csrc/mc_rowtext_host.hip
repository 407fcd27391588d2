// mc_rowtext_host.hip -- the rows of a pass as text, host side: the row writer of mc_rowtext.hip enqueued behind a pass's packed
// records, its pinned blocks handed out and taken back, and the probe of its numbers.  Host code only; the structures: mc_ctx.h.
#include "mc_ctx.h"

// The rows of a pass as text, made on the device behind its packed block (mc_rowtext.hip) and sent to a pinned block: for passes
// over a table the device parser made (the read names are in the shard's text), scored, with the context's classifier's key
// table.  Whatever is missing -- no free block, another kind of table -- leaves the pass without text: the host formats.
int mc_enqueue_row_text(mc_ctx *c, AsyncBuf &b, int64_t n, int64_t m, int64_t n_wide) {
    auto &R = c->rt;
    if (b.slot < 0 || m <= 0 || n <= 0 || !c->side_stream) { R.n_other += 1; return 0; }
    TableSlot &S = c->slots[b.slot];
    if (!S.from_parser || !S.text || !S.kp_segs || !S.kp_segs_h.p || !c->kc.chars || S.T.n_seg <= 0) { R.n_other += 1; return 0; }
    const uint8_t *soc = c->clf.sub_of_char;
    if (!soc || !b.prm.score || !b.qual || !c->R.seq) { R.n_other += 1; return 0; }
    hipStream_t st = c->side_stream;
    if (R.bytes_per_row <= 0.0) {
        size_t longest = 0;
        for (const std::string &nm : c->kc.names) longest = std::max(longest, nm.size());
        R.bytes_per_row = 64.0 + 2.0 * b.k + 20.0 * b.k + 64.0 + (double)longest;
    }
    const size_t need = (size_t)((double)m * R.bytes_per_row) + 4096;
    int at = -1;
    static const int n_blocks = getenv("MCALLER_ROW_TEXT_BLOCKS") ? std::max(0, std::min(MC_ROW_TEXT_BLOCKS, atoi(getenv("MCALLER_ROW_TEXT_BLOCKS")))) : MC_ROW_TEXT_BLOCKS;   // (tests: none free)
    for (int i = 0; i < n_blocks; ++i)
        if (R.blocks[i].busy.load() == 0 && (at < 0 || (R.blocks[at].cap < need && R.blocks[i].cap >= need))) at = i;
    if (at < 0) { R.n_no_block += 1; return 0; }
    auto &blk = R.blocks[at];
    if (blk.cap < need) {
        blk.cap = 0;
        const size_t cap = need + need / 4;
        if (blk.text.alloc(cap)) return -10;
        blk.cap = cap;
    }
    if (!blk.st.p) { if (blk.st.alloc(sizeof(RowTextStatus))) return -10; }
    if (R.out_cap < need) {
        HIP_TRY(hipStreamSynchronize(st));                  // (the row writer of the pass before may be at work in it)
        R.out_allocs.clear();
        R.out = nullptr; R.out_cap = 0;
        const size_t cap = need + need / 4;
        if (R.out_allocs.get(&R.out, cap)) return -10;
        R.out_cap = cap;
    }
    int64_t nbr, nbw;
    mc_row_text_scratch_sizes(n, m, &nbr, &nbw);
    if (R.cap_rec < n || R.cap_rows < m || R.cap_wide < n_wide || R.cap_num < n_wide + b.n_qual) {
        HIP_TRY(hipStreamSynchronize(st));
        R.allocs.clear();
        R.cap_rec = n + n / 4 + 1024; R.cap_rows = m + m / 4 + 1024;
        R.cap_wide = std::max<int64_t>(n_wide + n_wide / 4 + 1024, R.cap_wide);
        R.cap_num = std::max<int64_t>(R.cap_wide + b.n_qual + b.n_qual / 4 + 1024, R.cap_num);
        int64_t cbr, cbw;
        mc_row_text_scratch_sizes(R.cap_rec, R.cap_rows, &cbr, &cbw);
        if (R.allocs.get(&R.S.kept_blk, (size_t)cbr + 2) || R.allocs.get(&R.S.wide_blk, (size_t)cbw + 2) ||
            R.allocs.get(&R.S.wide_pref, (size_t)R.cap_rows) || R.allocs.get(&R.S.rec_len, (size_t)R.cap_rec) ||
            R.allocs.get(&R.S.rec_row, (size_t)R.cap_rec) || R.allocs.get(&R.S.len_blk, (size_t)cbr + 2) ||
            R.allocs.get(&R.S.wval, (size_t)R.cap_wide) || R.allocs.get(&R.S.num_lo, (size_t)R.cap_num) ||
            R.allocs.get(&R.S.num_meta, (size_t)R.cap_num) || R.allocs.get(&R.S.st, 1)) {
            R.cap_rec = R.cap_rows = R.cap_wide = R.cap_num = 0;
            return -10;
        }
    }
    const DevTable &T = S.T;
    RowTextIn I;
    I.pack = b.pack; I.n = n; I.m = m; I.n_wide = n_wide; I.k = b.k; I.close32 = b.close32 ? 1 : 0;
    I.seg_begin = T.seg_begin; I.seg_read = T.seg_read; I.seg_contig = T.seg_contig; I.n_seg = T.n_seg;
    I.segs = S.kp_segs; I.text = S.text;
    I.qual = b.qual; I.n_qual = b.n_qual;
    I.R = c->R;
    I.cn_off = c->kc.name_off; I.cn_len = c->kc.name_len; I.cn_chars = c->kc.chars;
    I.sub_of_char = soc;
    I.tail_contig = b.prm.tail_contig;
    memcpy(I.lab_meth, R.lab_meth, 8); memcpy(I.lab_unmeth, R.lab_unmeth, 8);
    I.lab_meth_len = R.lab_meth_len; I.lab_unmeth_len = R.lab_unmeth_len;
    // (the parser listed the segments as its lanes got there; the host's copy is in file order since mc_ctx_parse_end)
    if (int rc = mc_copy_by_kernel(S.kp_segs, S.kp_segs_h.p, (size_t)T.n_seg * sizeof(KpSeg), st)) return rc;
    mc_launch_row_text(I, R.S, R.out, R.room_forced ? std::min(need, std::min(R.out_cap, blk.cap)) : std::min(R.out_cap, blk.cap), (char *)blk.text.dev, (RowTextStatus *)blk.st.dev, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[EV_TEXT], st));
    R.next_ticket = R.next_ticket >= (1 << 24) ? 1 : R.next_ticket + 1;
    blk.busy.store(R.next_ticket);
    b.text_block = at;
    return 0;
}

// ---- rows of text made on the device ----
extern "C" int mc_ctx_row_text(mc_ctx *c, int32_t on, const char *label_meth, const char *label_unmeth) {
    auto &R = c->rt;
    if (on) {
        const size_t lm = label_meth ? strlen(label_meth) : 0, lu = label_unmeth ? strlen(label_unmeth) : 0;
        if (lm == 0 || lu == 0 || lm > 8 || lu > 8) {
            mc_set_error("mc_ctx_row_text: labels of 1..8 characters");
            return -12;
        }
        memset(R.lab_meth, 0, 8); memset(R.lab_unmeth, 0, 8);
        memcpy(R.lab_meth, label_meth, lm); memcpy(R.lab_unmeth, label_unmeth, lu);
        R.lab_meth_len = (int)lm; R.lab_unmeth_len = (int)lu;
        // on == 2, the first call of a stream: whatever held a block is gone (a stream that ended on an exception never gave its blocks
        // back).  Not on the later calls: with no pass in flight the host's writer may still be reading the blocks of the passes handed out
        if (on == 2 && c->ab_count == 0)
            for (auto &blk : R.blocks) blk.busy.store(0);
        R.room_forced = getenv("MCALLER_ROW_TEXT_ROOM") != nullptr;                                           // (tests: rows that do not fit)
        if (R.room_forced && !R.on) R.bytes_per_row = std::max(1.0, atof(getenv("MCALLER_ROW_TEXT_ROOM")));
    }
    if (!on && R.on && getenv("MCALLER_VERBOSE"))
        fprintf(stderr, "mcaller_hip: rows written on the device for %lld passes; not for %lld (no free block), %lld (a record for the host), %lld (room too small), %lld (other)\n",
                R.n_text, R.n_no_block, R.n_host_needed, R.n_too_small, R.n_other);
    R.on = on ? 1 : 0;
    return 0;
}

// (*block: the block's index and the ticket it was taken with -- a handle that has been given back, or that a later stream's first
// mc_ctx_row_text(2) declared void, frees nothing when it is given back again)
extern "C" int mc_last_row_text(mc_ctx *c, const char **text, int64_t *n_bytes, int64_t *n_rows, int32_t *block) {
    const auto &R = c->rt;
    *block = R.last_block >= 0 ? R.blocks[R.last_block].busy.load() * 8 + R.last_block : -1;
    *text = R.last_block >= 0 ? R.blocks[R.last_block].text.get<char>() : nullptr;
    *n_bytes = R.last_block >= 0 ? R.last_bytes : 0;
    *n_rows = R.last_block >= 0 ? R.last_rows : 0;
    return 0;
}

// (any thread: the host's writer gives a block back when the rows are in the file)
extern "C" int mc_row_text_release(mc_ctx *c, int32_t block) {
    if (block < 0 || (block & 7) >= MC_ROW_TEXT_BLOCKS) {
        mc_set_error("mc_row_text_release: no such block (%d)", block);
        return -12;
    }
    int ticket = block >> 3;
    if (ticket > 0) (void)c->rt.blocks[block & 7].busy.compare_exchange_strong(ticket, 0);     // (a stale handle: the block is somebody else's by now)
    return 0;
}

// the row writer's numbers alone (tests): the digit kernel and the sinks of mc_rowtext.hip on the caller's values
static int rowtext_probe(mc_ctx *c, Pool &pool, const double *v, int64_t n, const int32_t *fixed, int64_t n_fixed,
                         const double *prob, int64_t n_prob, int32_t shift, char *text, int32_t *len, uint8_t *ok) {
    const int64_t n_all = n + n_fixed + n_prob;
    const size_t text_bytes = (size_t)n_all * MC_ROWTEXT_PROBE_STRIDE;
    hipStream_t st = c->stream;
    RowTextScratch S = {};
    double *d_q = nullptr, *d_prob = nullptr;
    int32_t *d_fixed = nullptr, *d_len = nullptr;
    uint8_t *d_ok = nullptr;
    char *d_text = nullptr;
    if (pool.get(&S.wval, (size_t)n) || pool.get(&d_q, (size_t)n) || pool.get(&S.num_lo, (size_t)n) ||
        pool.get(&S.num_meta, (size_t)n) || pool.get(&d_fixed, (size_t)n_fixed) || pool.get(&d_prob, (size_t)n_prob) ||
        pool.get(&d_text, text_bytes) || pool.get(&d_len, (size_t)n_all) || pool.get(&d_ok, (size_t)n_all))
        return -10;
    RowTextIn I = {};
    I.n_wide = n / 2;                                   // the first half as wide slot means, the rest as read qualities (k_rt_digits' two sources)
    I.n_qual = (int32_t)(n - n / 2);
    I.qual = d_q;
    if (I.n_wide) HIP_TRY(hipMemcpyAsync(S.wval, v, (size_t)I.n_wide * 8, hipMemcpyHostToDevice, st));
    if (I.n_qual) HIP_TRY(hipMemcpyAsync(d_q, v + I.n_wide, (size_t)I.n_qual * 8, hipMemcpyHostToDevice, st));
    if (n_fixed) HIP_TRY(hipMemcpyAsync(d_fixed, fixed, (size_t)n_fixed * 4, hipMemcpyHostToDevice, st));
    if (n_prob) HIP_TRY(hipMemcpyAsync(d_prob, prob, (size_t)n_prob * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_text, 0xA5, text_bytes, st));
    mc_launch_row_text_probe(I, S, d_fixed, n_fixed, d_prob, n_prob, shift, d_text, d_len, d_ok, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(text, d_text, text_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(len, d_len, (size_t)n_all * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ok, d_ok, (size_t)n_all, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mc_ctx_rowtext_probe(mc_ctx *c, const double *v, int64_t n, const int32_t *fixed, int64_t n_fixed, const double *prob,
                                    int64_t n_prob, int32_t shift, char *text, int32_t *len, uint8_t *ok) {
    HIP_TRY(hipSetDevice(c->device));
    if (n < 0 || n_fixed < 0 || n_prob < 0 || shift < 0 || n - n / 2 > INT32_MAX) {
        mc_set_error("mc_ctx_rowtext_probe: counts and shift >= 0");
        return -12;
    }
    if (n + n_fixed + n_prob == 0) return 0;
    Pool pool("mc_ctx_rowtext_probe");
    const int rc = rowtext_probe(c, pool, v, n, fixed, n_fixed, prob, n_prob, shift, text, len, ok);
    if (rc) (void)hipStreamSynchronize(c->stream);      // (nothing may still be writing into what the pool frees)
    return rc;
}
