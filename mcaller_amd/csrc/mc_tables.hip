// mc_tables.hip -- table slots (uploads, select, fetch), the host side of the device parser and the reference setters: the one
// unit that includes mc_devparse.inc, whose kernels (kp_*, k_mark_*, k_ref_planes, k_copy_bytes) sit in an unnamed namespace.  The structures:
// mc_ctx.h.
#include "mc_ctx.h"
#include "mc_iupac.h"

static SmallLayout small_layout(int64_t n_seg, int64_t n_tiles, int64_t n_reads) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    SmallLayout L;
    size_t o = 0;
    L.seg_begin = o;    o = al(o + (size_t)(n_seg + 1) * 8);
    L.seg_read = o;     o = al(o + (size_t)n_seg * 4);
    L.seg_contig = o;   o = al(o + (size_t)n_seg * 4);
    L.nb_row_begin = o; o = al(o + (size_t)(n_seg + 1) * 8);
    L.nb_seg_begin = o; o = al(o + (size_t)(n_seg + 1) * 4);
    L.nb_read = o;      o = al(o + (size_t)n_seg * 4);
    L.nb_repeat = o;    o = al(o + (size_t)n_seg);
    L.nb_vflags = o;    o = al(o + (size_t)(n_seg + 1) * 4);
    L.tile_nb = o;      o = al(o + (size_t)(n_tiles + 1) * 4);
    L.qual = o;         o = al(o + (size_t)n_reads * 8);
    L.total = o;
    return L;
}

#include "mc_devparse.inc"

// dst / src: device memory or pinned host memory (hipHostMalloc), both 16-byte aligned
int mc_copy_by_kernel(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return 0;
    void *d = dst;
    const void *s = src;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, dst) == hipSuccess && a.type == hipMemoryTypeHost) HIP_TRY(hipHostGetDevicePointer(&d, dst, 0));
    else (void)hipGetLastError();
    if (hipPointerGetAttributes(&a, src) == hipSuccess && a.type == hipMemoryTypeHost) HIP_TRY(hipHostGetDevicePointer((void **)&s, const_cast<void *>(src), 0));
    else (void)hipGetLastError();
    const unsigned blocks = (unsigned)std::min<size_t>((bytes / 16 + 255) / 256 + 1, 1024);
    hipLaunchKernelGGL(k_copy_bytes, dim3(blocks), dim3(256), 0, st, (unsigned char *)d, (const unsigned char *)s, bytes);
    return 0;
}

// What both reference setters begin with: the streams that read the reference are drained (passes in flight read it; the text
// uploads and the device parser do not), the old one is released, the new one's contigs are counted
static int begin_reference(mc_ctx *c, const mc_ref_view *h) {
    if (c->side_stream) HIP_TRY(hipStreamSynchronize(c->side_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream2));
    c->ref_version += 1;                                   // the name-block templates of every slot are stale
    c->ref_allocs.clear();
    c->R.n_contigs = h->n_contigs;
    c->ref_total_len = 0;
    for (int32_t ci = 0; ci < h->n_contigs; ++ci) c->ref_total_len += h->contig_len[ci];
    return 0;
}

// ... and end with: the site counts of the old reference's numbering go
static void end_reference(mc_ctx *c) {
    if (c->site_stream) (void)hipStreamSynchronize(c->site_stream);
    c->site_allocs.clear();
    c->site_cnt = nullptr; c->site_first = nullptr; c->site_n = 0;
}

extern "C" int mc_ctx_set_reference(mc_ctx *c, const mc_ref_view *h) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = begin_reference(c, h)) return rc;
    DevRef &R = c->R;
    // site numbers: per contig, all '+' sites then all '-' sites, ascending position
    std::vector<int32_t> rank_f((size_t)h->n_words + 1), rank_r((size_t)h->n_words + 1);
    std::vector<int64_t> base((size_t)h->n_contigs * 2 + 2);
    int64_t n_sites = 0;
    for (int32_t ci = 0; ci < h->n_contigs; ++ci) {
        const int64_t w0 = h->word_off[ci], w1 = ci + 1 < h->n_contigs ? h->word_off[ci + 1] : h->n_words;
        for (int st = 0; st < 2; ++st) {
            const uint32_t *bits = st ? h->mbits_rev : h->mbits_fwd;
            std::vector<int32_t> &rank = st ? rank_r : rank_f;
            base[(size_t)ci * 2 + st] = n_sites;
            int32_t run = 0;
            for (int64_t w = w0; w < w1; ++w) {
                rank[(size_t)w] = run;
                run += __builtin_popcount(bits[w]);
            }
            n_sites += run;
        }
    }
    R.n_sites = n_sites;
    // Everything goes through ONE pinned stage and is moved by a kernel: while a file is streamed the DMA engines are busy
    // with the text of the shards ahead, and a transfer submitted now would complete behind all of them (k_copy_bytes).
    struct Piece { void **dev; const void *src; size_t bytes, off; };
    size_t total = 0;
    auto piece = [&](void **dev, const void *src, size_t bytes) { Piece p{dev, src, bytes, total}; total += (bytes + 255) & ~(size_t)255; return p; };
    Piece pieces[] = {
        piece((void **)&R.contig_len, h->contig_len, (size_t)h->n_contigs * 8), piece((void **)&R.seq_off, h->seq_off, (size_t)h->n_contigs * 8),
        piece((void **)&R.word_off, h->word_off, (size_t)h->n_contigs * 8), piece((void **)&R.seq, h->seq, (size_t)h->n_seq_bytes),
        piece((void **)&R.mf, h->mbits_fwd, (size_t)h->n_words * 4), piece((void **)&R.mr, h->mbits_rev, (size_t)h->n_words * 4),
        piece((void **)&R.rank_f, rank_f.data(), (size_t)h->n_words * 4), piece((void **)&R.rank_r, rank_r.data(), (size_t)h->n_words * 4),
        piece((void **)&R.site_base, base.data(), (size_t)h->n_contigs * 2 * 8)};
    unsigned char *dev_block = nullptr;
    Pinned stage_pin;
    if (c->ref_allocs.get(&dev_block, total + 256) || stage_pin.alloc(total + 256)) return -10;
    unsigned char *stage = stage_pin.get<unsigned char>();
    for (const Piece &p : pieces) {
        if (p.bytes) memcpy(stage + p.off, p.src, p.bytes);
        *p.dev = dev_block + p.off;
    }
    int rc = mc_copy_by_kernel(dev_block, stage, total, c->stream);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) { mc_set_error("mc_ctx_set_reference: the upload failed"); rc = -11; }
    if (rc) return rc;
    end_reference(c);
    return 0;
}

// The reference from its raw bases, the masks made on the device (k_mark_*): h->seq holds the FASTA bytes of every contig
// (any case), h->mbits_* are not read.  *_fwd: the motif and what str.replace puts in its place for the '+' strand, *_rev: for
// the reverse complement; the motifs must not be able to overlap themselves (the caller checks; a one-base motif cannot).
extern "C" int mc_ctx_set_reference_motif(mc_ctx *c, const mc_ref_view *h, const char *motif_fwd, const char *repl_fwd, int32_t m_fwd,
                                          const char *motif_rev, const char *repl_rev, int32_t m_rev) {
    HIP_TRY(hipSetDevice(c->device));
    if (!h || h->n_contigs < 1 || !h->seq || m_fwd < 1 || m_fwd > 16 || m_rev < 1 || m_rev > 16 || !motif_fwd || !repl_fwd || !motif_rev ||
        !repl_rev || h->n_words < 1) {
        mc_set_error("mc_ctx_set_reference_motif: bad arguments (motifs of 1..16 bases)");
        return -12;
    }
    if (int rc = begin_reference(c, h)) return rc;
    DevRef &R = c->R;
    MarkMotif F, Rv;
    memset(&F, 0, sizeof(F)); memset(&Rv, 0, sizeof(Rv));
    memcpy(F.motif, motif_fwd, (size_t)m_fwd); memcpy(F.repl, repl_fwd, (size_t)m_fwd); F.m = m_fwd;
    memcpy(Rv.motif, motif_rev, (size_t)m_rev); memcpy(Rv.repl, repl_rev, (size_t)m_rev); Rv.m = m_rev;
    // one pinned stage for the small arrays and the bases, moved by a kernel (see mc_ctx_set_reference)
    const size_t nc = (size_t)h->n_contigs, nb = (size_t)h->n_seq_bytes, nw = (size_t)h->n_words;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_len = 0, o_soff = al(nc * 8), o_woff = o_soff + al(nc * 8), o_raw = o_woff + al(nc * 8), in_total = o_raw + al(nb + 16);
    unsigned char *dev_in = nullptr;
    uint8_t *seq = nullptr;
    long long *cnt = nullptr, *off = nullptr, *total = nullptr;
    Pool tmp("mc_ctx_set_reference_motif");                  // scratch of this call
    Pinned stage_pin;
    if (c->ref_allocs.get(&dev_in, in_total) || c->ref_allocs.get(&seq, nb + 16) || c->ref_allocs.get(&R.mf, nw) ||
        c->ref_allocs.get(&R.mr, nw) || c->ref_allocs.get(&R.rank_f, nw) || c->ref_allocs.get(&R.rank_r, nw) ||
        c->ref_allocs.get(&R.site_base, nc * 2) || tmp.get(&cnt, 2 * nw + 1) || tmp.get(&off, 2 * nw + 1) ||
        tmp.get(&total, 1) || stage_pin.alloc(in_total))
        return -10;
    unsigned char *stage = stage_pin.get<unsigned char>();
    memcpy(stage + o_len, h->contig_len, nc * 8);
    memcpy(stage + o_soff, h->seq_off, nc * 8);
    memcpy(stage + o_woff, h->word_off, nc * 8);
    memcpy(stage + o_raw, h->seq, nb);
    memset(stage + o_raw + nb, 0, 16);
    R.contig_len = (int64_t *)(dev_in + o_len); R.seq_off = (int64_t *)(dev_in + o_soff); R.word_off = (int64_t *)(dev_in + o_woff);
    R.seq = seq;
    hipStream_t st = c->stream;
    int rc = mc_copy_by_kernel(dev_in, stage, in_total, st);
    if (!rc) {
        hipLaunchKernelGGL(k_mark_upper, dim3(1024), dim3(256), 0, st, (const uint8_t *)(dev_in + o_raw), seq, (int64_t)nb + 16);
        const unsigned wb = (unsigned)((nw + 255) / 256);
        hipLaunchKernelGGL(k_mark_words, dim3(wb), dim3(256), 0, st, (const uint8_t *)seq, (const int64_t *)R.contig_len,
                           (const int64_t *)R.seq_off, (const int64_t *)R.word_off, h->n_contigs, (int64_t)nw, F, Rv, R.mf, R.mr, cnt);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)cnt, (int64_t)(2 * nw), off, total);
        hipLaunchKernelGGL(k_mark_ranks, dim3(wb), dim3(256), 0, st, (const long long *)off, (const int64_t *)R.word_off, h->n_contigs,
                           (int64_t)nw, R.rank_f, R.rank_r, R.site_base);
        long long n_sites = 0;
        if (hipMemcpyAsync(&n_sites, total, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            mc_set_error("mc_ctx_set_reference_motif: the marking failed: %s", hipGetErrorString(hipGetLastError()));
            rc = -11;
        }
        R.n_sites = n_sites;
    }
    if (rc) return rc;
    end_reference(c);
    return 0;
}

// The reference from its raw bases for a set of degenerate motifs (mc_iupac.h), the masks made on the device: k_ref_planes turns
// the bases into bit-planes, k_mark_iupac matches every motif of both strands on them.  The same staging and the same results as
// mc_ctx_set_reference_motif: R.seq upper-cased, R.mf / R.mr, the site numbering.
extern "C" int mc_ctx_set_reference_iupac(mc_ctx *c, const mc_ref_view *h, const mc_iupac_spec *spec) {
    HIP_TRY(hipSetDevice(c->device));
    bool ok = h && h->n_contigs >= 1 && h->seq && h->n_words >= 1 && h->n_seq_bytes >= 0 && iu_spec_ok(spec);
    // (the kernels index by this layout: every contig's bases inside seq, its mask words -- two of padding -- inside the grid)
    for (int32_t ci = 0; ok && ci < h->n_contigs; ++ci) {
        const int64_t L = h->contig_len[ci], w0 = h->word_off[ci], w1 = ci + 1 < h->n_contigs ? h->word_off[ci + 1] : h->n_words;
        ok = L >= 0 && h->seq_off[ci] >= 0 && h->seq_off[ci] <= h->n_seq_bytes - L && w0 >= 0 && (ci > 0 || w0 == 0) &&
             w1 - w0 >= (L + 31) / 32 + 2 && w1 <= h->n_words;
    }
    if (!ok) {
        mc_set_error("mc_ctx_set_reference_iupac: bad arguments (1..%d motifs of 1..%d letters; ceil(len / 32) + 2 mask words per contig)",
                     MC_IUPAC_MAX_MOTIFS, MC_IUPAC_MAX_LEN);
        return -12;
    }
    if (int rc = begin_reference(c, h)) return rc;
    DevRef &R = c->R;
    // one pinned stage for the small arrays and the bases, moved by a kernel (see mc_ctx_set_reference)
    const size_t nc = (size_t)h->n_contigs, nb = (size_t)h->n_seq_bytes, nw = (size_t)h->n_words;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_len = 0, o_soff = al(nc * 8), o_woff = o_soff + al(nc * 8), o_raw = o_woff + al(nc * 8), in_total = o_raw + al(nb + 16);
    unsigned char *dev_in = nullptr;
    uint8_t *seq = nullptr;
    uint32_t *planes = nullptr;
    long long *cnt = nullptr, *off = nullptr, *total = nullptr;
    Pool tmp("mc_ctx_set_reference_iupac");                  // scratch of this call
    Pinned stage_pin;
    if (c->ref_allocs.get(&dev_in, in_total) || c->ref_allocs.get(&seq, nb + 16) || c->ref_allocs.get(&R.mf, nw) ||
        c->ref_allocs.get(&R.mr, nw) || c->ref_allocs.get(&R.rank_f, nw) || c->ref_allocs.get(&R.rank_r, nw) ||
        c->ref_allocs.get(&R.site_base, nc * 2) || tmp.get(&planes, (size_t)IU_PLANES * nw) || tmp.get(&cnt, 2 * nw + 1) ||
        tmp.get(&off, 2 * nw + 1) || tmp.get(&total, 1) || stage_pin.alloc(in_total))
        return -10;
    unsigned char *stage = stage_pin.get<unsigned char>();
    memcpy(stage + o_len, h->contig_len, nc * 8);
    memcpy(stage + o_soff, h->seq_off, nc * 8);
    memcpy(stage + o_woff, h->word_off, nc * 8);
    memcpy(stage + o_raw, h->seq, nb);
    memset(stage + o_raw + nb, 0, 16);
    R.contig_len = (int64_t *)(dev_in + o_len); R.seq_off = (int64_t *)(dev_in + o_soff); R.word_off = (int64_t *)(dev_in + o_woff);
    R.seq = seq;
    hipStream_t st = c->stream;
    int rc = mc_copy_by_kernel(dev_in, stage, in_total, st);
    if (!rc) {
        // (bytes of seq that belong to no contig, and the 16 behind the last one: upper-cased as they are)
        hipLaunchKernelGGL(k_mark_upper, dim3(1024), dim3(256), 0, st, (const uint8_t *)(dev_in + o_raw), seq, (int64_t)nb + 16);
        const unsigned pb = (unsigned)std::min<size_t>(((nw + 1) / 2 + 3) / 4, 4096);      // (four waves a block, 64 bases a wave and step)
        hipLaunchKernelGGL(k_ref_planes, dim3(pb), dim3(256), 0, st, (const uint8_t *)(dev_in + o_raw), seq, (const int64_t *)R.contig_len,
                           (const int64_t *)R.seq_off, (const int64_t *)R.word_off, h->n_contigs, (int64_t)nw, planes);
        const unsigned wb = (unsigned)((nw + 255) / 256);
        hipLaunchKernelGGL(k_mark_iupac, dim3(wb), dim3(256), 0, st, (const uint32_t *)planes, (const int64_t *)R.word_off, h->n_contigs,
                           (int64_t)nw, *spec, R.mf, R.mr, cnt);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)cnt, (int64_t)(2 * nw), off, total);
        hipLaunchKernelGGL(k_mark_ranks, dim3(wb), dim3(256), 0, st, (const long long *)off, (const int64_t *)R.word_off, h->n_contigs,
                           (int64_t)nw, R.rank_f, R.rank_r, R.site_base);
        long long n_sites = 0;
        if (hipMemcpyAsync(&n_sites, total, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            mc_set_error("mc_ctx_set_reference_iupac: the marking failed: %s", hipGetErrorString(hipGetLastError()));
            rc = -11;
        }
        R.n_sites = n_sites;
    }
    if (rc) return rc;
    end_reference(c);
    return 0;
}

// the reference as the device holds it, back on the host (tests: the masks made on the device against the host's marking)
extern "C" int mc_ctx_fetch_reference(mc_ctx *c, uint8_t *seq, int64_t n_seq_bytes, uint32_t *mbits_fwd, uint32_t *mbits_rev, int32_t *rank_fwd,
                                      int32_t *rank_rev, int64_t n_words, int64_t *site_base, int64_t *n_sites) {
    HIP_TRY(hipSetDevice(c->device));
    const DevRef &R = c->R;
    if (!R.seq || !R.mf) {
        mc_set_error("mc_ctx_fetch_reference: no reference set");
        return -12;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (seq) HIP_TRY(hipMemcpy(seq, R.seq, (size_t)n_seq_bytes, hipMemcpyDeviceToHost));
    if (mbits_fwd) HIP_TRY(hipMemcpy(mbits_fwd, R.mf, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    if (mbits_rev) HIP_TRY(hipMemcpy(mbits_rev, R.mr, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    if (rank_fwd) HIP_TRY(hipMemcpy(rank_fwd, R.rank_f, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    if (rank_rev) HIP_TRY(hipMemcpy(rank_rev, R.rank_r, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    if (site_base) HIP_TRY(hipMemcpy(site_base, R.site_base, (size_t)R.n_contigs * 16, hipMemcpyDeviceToHost));
    if (n_sites) *n_sites = R.n_sites;
    return 0;
}

// ---- table slots ----
static void slot_free_parser(TableSlot &S) {
    S.kp_allocs.clear();
    for (Pinned *p : {&S.kp_head_h, &S.kp_segs_h, &S.kp_unknown_h, &S.kp_flags_h}) p->reset();
    S.text = nullptr; S.cap_text = 0; S.kp_head = nullptr; S.kp_segs = nullptr;
    S.kp_unknown = nullptr; S.kp_cap_flags = 0; S.kp_cap_segs = 0; S.kp_state = 0;
}

static void slot_free(TableSlot &S) {
    S.allocs.clear();
    slot_free_parser(S);
    S.stage.reset();
    S.nbits_h.reset();
    S.xrel_h.reset();
    S.small_dev = nullptr;
    S.pos = S.idx = nullptr; S.evmu = nullptr; S.flags = nullptr; S.nbits = nullptr; S.xrel = nullptr; S.prel = nullptr; S.nb_tmpl = nullptr; S.unit_pp = nullptr;
    S.cap_rows = S.cap_segs = S.cap_reads = 0;
    S.T = DevTable();
    S.qual = nullptr; S.n_qual = 0; S.tmpl_ref = -1;
}

// device memory + pinned stage of a slot for tables of up to (rows, segs, reads)
static int slot_ensure(mc_ctx *c, TableSlot &S, int64_t rows, int64_t segs, int64_t reads) {
    if (!S.ev_uploaded) {
        for (Event *e : {&S.ev_uploaded, &S.ev_up_start, &S.ev_val_start, &S.ev_valid})
            if (int rc = e->create()) return rc;
        HIP_TRY(hipEventRecord(S.ev_valid, c->stream));           // (so that the first upload has something to wait for)
    }
    if (S.pos && rows <= S.cap_rows && segs <= S.cap_segs && reads <= S.cap_reads) return 0;
    // growing: whatever may still read the old arrays has to finish first (only ever happens without mc_ctx_reserve_tables)
    if (int rc = mc_sync_pass_streams(c)) return rc;
    const bool fresh = !S.pos;
    slot_free(S);
    auto grow = [&](int64_t need, int64_t reserved) { return std::max<int64_t>(fresh ? need : need + need / 4, reserved); };
    S.cap_rows = grow(rows, c->res_rows);
    S.cap_segs = std::max<int64_t>(grow(segs, c->res_segs), 16);
    S.cap_reads = std::max<int64_t>(grow(reads, c->res_reads), 16);
    const int64_t padded = ((S.cap_rows + TILE - 1) / TILE) * TILE + TILE + FRONT;     // (whole tiles of the scan)
    const SmallLayout L = small_layout(S.cap_segs, padded / TILE, S.cap_reads);
    if (S.allocs.get(&S.pos, (size_t)padded) || S.allocs.get(&S.idx, (size_t)padded) ||
        S.allocs.get(&S.evmu, (size_t)padded) || S.allocs.get(&S.flags, (size_t)padded) ||
        S.allocs.get(&S.unit_pp, (size_t)padded / 8 + 8) || S.allocs.get(&S.nbits, (size_t)padded / 8 + 8) ||
        S.allocs.get(&S.xrel, (size_t)padded / 8 + 8) || S.allocs.get(&S.prel, (size_t)padded / 8 + 8))
        return -10;
    // (FRONT rows of padding before row 0 of the columns k1_emit looks back into: rows -1 .. -64 are readable; nothing looks
    // back through the bit column, which like the others reaches a tile beyond the table's last whole tile)
    S.pos += FRONT; S.evmu += FRONT; S.flags += FRONT;
    if (
        S.allocs.get(&S.nb_tmpl, (size_t)S.cap_segs + 1) || S.allocs.get(&S.small_dev, L.total))
        return -10;
    if (int rc = S.stage.alloc(L.total)) return rc;
    return 0;
}

extern "C" int mc_ctx_reserve_tables(mc_ctx *c, int64_t max_rows, int32_t max_segs, int32_t max_reads) {
    HIP_TRY(hipSetDevice(c->device));
    if (max_rows < 0 || max_segs < 0 || max_reads < 0) {
        mc_set_error("mc_ctx_reserve_tables: negative size");
        return -12;
    }
    c->res_rows = std::max(c->res_rows, max_rows);
    c->res_segs = std::max<int64_t>(c->res_segs, max_segs);
    c->res_reads = std::max<int64_t>(c->res_reads, max_reads);
    for (TableSlot &S : c->slots)
        if (int rc = slot_ensure(c, S, c->res_rows, c->res_segs, c->res_reads)) return rc;
    return mc_ensure_scratch(c, c->res_segs, (c->res_rows + TILE - 1) / TILE);
}

// a free slot: not scanned by a pass in flight, not holding the records handed out last, not being filled by the device parser
static int free_slot(mc_ctx *c, const char *who) {
    for (int i = 1; i <= MC_TABLE_SLOTS; ++i) {
        const int sidx = (std::max(c->cur, 0) + i) % MC_TABLE_SLOTS;
        if (c->slots[sidx].refs == 0 && sidx != c->held) return sidx;
    }
    mc_set_error("%s: all %d table slots are being scanned; call mc_wait_records first", who, MC_TABLE_SLOTS);
    return -1;
}

// What makes the rows in slot `at` a table: the small arrays (segments, name blocks -- maximal runs of segments with one read
// name --, the name block of every tile's first row, read qualities) laid out in the pinned stage and sent, the per-table
// kernel behind them; the table becomes the current one.  cols: the host columns to send first (mc_ctx_upload_table_async),
// or nullptr: the device parser has put them into the slot already (mc_ctx_parse_finish).  seg_name_start[sg] (or, if
// nullptr, MC_F_NAME_START of the segment's first row in cols->flags): the segment starts a name block.
static int fill_slot(mc_ctx *c, int at, int64_t n, int32_t n_seg, const int64_t *seg_row_begin, const int32_t *seg_read_in,
                     const int32_t *seg_contig_in, const uint8_t *seg_name_start, int32_t n_reads, const double *read_qual,
                     const mc_table_view *cols) {
    TableSlot &S = c->slots[at];
    S.from_parser = cols == nullptr;
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    const SmallLayout L = small_layout(n_seg, n_tiles, read_qual ? n_reads : 0);
    unsigned char *st = S.stage.get<unsigned char>();
    int64_t *seg_begin = (int64_t *)(st + L.seg_begin), *nb_row = (int64_t *)(st + L.nb_row_begin);
    int32_t *seg_read = (int32_t *)(st + L.seg_read), *seg_contig = (int32_t *)(st + L.seg_contig);
    int32_t *nb_seg = (int32_t *)(st + L.nb_seg_begin), *nb_read = (int32_t *)(st + L.nb_read), *tile_nb = (int32_t *)(st + L.tile_nb);
    uint8_t *nb_rep = st + L.nb_repeat;
    uint32_t *nb_vf = (uint32_t *)(st + L.nb_vflags);
    if (n_seg > 0) {
        memcpy(seg_begin, seg_row_begin, (size_t)n_seg * 8);
        seg_begin[n_seg] = n;
        memcpy(seg_read, seg_read_in, (size_t)n_seg * 4);
        memcpy(seg_contig, seg_contig_in, (size_t)n_seg * 4);
    } else seg_begin[0] = 0;
    std::vector<uint8_t> seen((size_t)std::max(n_reads, 1), 0);
    int has_rep = 0;
    int32_t n_nb = 0;
    for (int32_t sg = 0; sg < n_seg; ++sg) {
        const int64_t rb = seg_row_begin[sg];
        if (rb < 0 || rb >= n || (sg > 0 && rb <= seg_row_begin[sg - 1])) {
            mc_set_error("segment %d: row %lld out of order", sg, (long long)rb);
            return -12;
        }
        if (sg == 0 || (seg_name_start ? seg_name_start[sg] != 0 : (cols->flags[rb] & MC_F_NAME_START) != 0)) {
            const int32_t rd = seg_read_in[sg];
            if (rd < 0 || rd >= n_reads) {
                mc_set_error("segment %d: read id %d out of range", sg, rd);
                return -12;
            }
            nb_row[n_nb] = rb;
            nb_seg[n_nb] = sg;
            nb_read[n_nb] = rd;
            nb_rep[n_nb] = seen[(size_t)rd];
            has_rep |= seen[(size_t)rd];
            seen[(size_t)rd] = 1;
            if (n_nb > 0) nb_vf[n_nb - 1] = (sg - nb_seg[n_nb - 1] > 1) ? V_MULTI_SEG : 0u;
            ++n_nb;
        }
    }
    if (n_nb > 0) nb_vf[n_nb - 1] = (n_seg - nb_seg[n_nb - 1] > 1) ? V_MULTI_SEG : 0u;
    nb_row[n_nb] = n;
    nb_seg[n_nb] = n_seg;
    nb_vf[n_nb] = 0u;
    {
        int32_t b = 0;                                     // last block that starts at or before the tile's first row
        for (int64_t t = 0; t < n_tiles; ++t) {
            while (b + 1 < n_nb && nb_row[b + 1] <= t * TILE) ++b;
            tile_nb[t] = b;
        }
    }
    if (read_qual && n_reads > 0) memcpy(st + L.qual, read_qual, (size_t)n_reads * 8);

    // ---- the slot's table ----
    DevTable &T = S.T;
    T = DevTable();
    T.n_rows = n; T.n_seg = n_seg; T.n_reads = n_reads; T.n_nb = n_nb; T.n_tiles = n_tiles; T.has_repeats = has_rep;
    T.pos = S.pos; T.idx = S.idx; T.evmu = S.evmu; T.flags = S.flags; T.nbits = S.nbits; T.xrel = S.xrel; T.prel = S.prel; T.nb_tmpl = S.nb_tmpl; T.unit_pp = S.unit_pp;
    unsigned char *dv = S.small_dev;
    T.seg_begin = (int64_t *)(dv + L.seg_begin); T.seg_read = (int32_t *)(dv + L.seg_read); T.seg_contig = (int32_t *)(dv + L.seg_contig);
    T.nb_row_begin = (int64_t *)(dv + L.nb_row_begin); T.nb_seg_begin = (int32_t *)(dv + L.nb_seg_begin);
    T.nb_read = (int32_t *)(dv + L.nb_read); T.nb_repeat = dv + L.nb_repeat; T.nb_vflags = (uint32_t *)(dv + L.nb_vflags);
    T.tile_nb = (int32_t *)(dv + L.tile_nb);
    S.qual = read_qual ? (double *)(dv + L.qual) : nullptr;
    S.n_qual = read_qual ? n_reads : 0;
    S.tmpl_ref = -1;
    S.passes = 0;                                          // (the first pass over these rows validates them)
    S.summarized = n > 0;                                  // (kp_place wrote unit_pp and prel with the columns; k_unit_columns below)

    // ---- H2D on the upload stream (nothing reads the slot: its passes have been handed out); the ctx stream waits for the
    //      transfer ----
    // (a device-parsed table: the upload stream is busy with the NEXT shard's text by now -- the small arrays go on the ctx
    // stream, in front of the kernels that read them)
    hipStream_t us = cols ? c->up_stream : c->stream;
    if (cols) {
        HIP_TRY(hipStreamWaitEvent(us, S.ev_valid, 0));    // the small arrays of the slot's previous table (it may never have been scanned)
        HIP_TRY(hipEventRecord(S.ev_up_start, us));
        if (n > 0) {
            HIP_TRY(hipMemcpyAsync(T.pos, cols->pos, (size_t)n * 4, hipMemcpyHostToDevice, us));
            HIP_TRY(hipMemcpyAsync(T.evmu, cols->event_model_e4, (size_t)n * 8, hipMemcpyHostToDevice, us));
            HIP_TRY(hipMemcpyAsync(T.idx, cols->event_idx, (size_t)n * 4, hipMemcpyHostToDevice, us));
            HIP_TRY(hipMemcpyAsync(T.flags, cols->flags, (size_t)n, hipMemcpyHostToDevice, us));
            // the model-N bits: the caller's column, or packed here for one that has none (bare arrays: one pass of the host
            // over the flags; the slot's pinned block is free -- the transfers of the slot's previous table have been waited for)
            const uint8_t *nbits = cols->model_n_bits;
            if (!nbits) {
                if (!S.nbits_h.p) { if (int rc = S.nbits_h.alloc((size_t)(S.cap_rows + 7) / 8 + 8)) return rc; }       // (freed when the slot grows)
                mc_pack_model_n(cols->flags, n, S.nbits_h.get<uint8_t>());
                nbits = S.nbits_h.get<uint8_t>();
            }
            HIP_TRY(hipMemcpyAsync(T.nbits, nbits, (size_t)(n + 7) / 8, hipMemcpyHostToDevice, us));
            // the index relations, likewise: the caller's column, or one pass of the host over the indices into the slot's block
            const uint16_t *xrel = cols->idx_rel_bits;
            if (!xrel) {
                if (!S.xrel_h.p) { if (int rc = S.xrel_h.alloc(((size_t)(S.cap_rows + 7) / 8 + 8) * 2)) return rc; }       // (freed when the slot grows)
                mc_pack_idx_rel(cols->event_idx, n, S.xrel_h.get<uint16_t>());
                xrel = S.xrel_h.get<uint16_t>();
            }
            HIP_TRY(hipMemcpyAsync(T.xrel, xrel, (size_t)(n + 7) / 8 * 2, hipMemcpyHostToDevice, us));
            // the unit summaries and the position relations: made on the device from the position column that has just arrived
            // (one read of 4 B/row from HBM behind 17.4 B/row over the link; nothing more to pack, pin or send)
            mc_launch_unit_columns(T, us);
        }
    }
    if (!cols && L.total <= COPY_BY_KERNEL_MAX) { if (int rc = mc_copy_by_kernel(dv, st, L.total, us)) return rc; }     // (not behind the next shard's text)
    else HIP_TRY(hipMemcpyAsync(dv, st, L.total, hipMemcpyHostToDevice, us));
    HIP_TRY(hipEventRecord(S.ev_uploaded, us));
    HIP_TRY(hipStreamWaitEvent(c->stream, S.ev_uploaded, 0));
    HIP_TRY(hipEventRecord(S.ev_val_start, c->stream));
    HIP_TRY(hipEventRecord(S.ev_valid, c->stream));
    HIP_TRY(hipGetLastError());
    c->T = T;
    c->cur = at;
    S.holds_table = true;
    if (read_qual) { c->qual = S.qual; c->n_qual = S.n_qual; }
    else { c->qual = c->qual_own; c->n_qual = c->n_qual_own; }       // mc_ctx_set_read_quality's table applies
    return 0;
}

extern "C" int mc_ctx_upload_table_async(mc_ctx *c, const mc_table_view *h, const double *read_qual, int32_t *slot_out) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot_out) *slot_out = -1;
    const int64_t n = h->n_rows;
    if (n < 0 || h->n_seg < 0 || h->n_reads < 0 || (n > 0 && h->n_seg == 0)) {
        mc_set_error("mc_ctx_upload_table_async: malformed table (%lld rows, %d segments, %d reads)", (long long)n, h->n_seg, h->n_reads);
        return -12;
    }
    const int at = free_slot(c, "mc_ctx_upload_table_async");
    if (at < 0) return MC_E_NO_FREE_SLOT;
    TableSlot &S = c->slots[at];
    if (int rc = slot_ensure(c, S, n, h->n_seg, h->n_reads)) return rc;
    HIP_TRY(hipEventSynchronize(S.ev_uploaded));          // the stage is about to be rewritten (long done: the slot was idle)
    if (int rc = fill_slot(c, at, n, h->n_seg, h->seg_row_begin, h->seg_read, h->seg_contig, nullptr, h->n_reads, read_qual, h)) return rc;
    if (slot_out) *slot_out = at;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The device parser's host side (kernels: mc_devparse.inc).  mc_ctx_parse_begin sends a shard's text and enqueues the
// kernels that turn it into the columns of a table slot; mc_ctx_parse_end waits and hands out what the host needs to name
// things (segments with the place of their read name in the text, unknown contig tokens, the flag column);
// mc_ctx_parse_finish takes the read ids and qualities and makes the slot's rows the current table -- from there on the slot
// is what mc_ctx_upload_table_async would have left.  All on the upload stream; begin for shard i+1 may be called before end
// for shard i.
// ---------------------------------------------------------------------------------------------------
static int kp_ensure_scratch(mc_ctx *c, int64_t cap_lines, int64_t n_tiles) {
    KpScratch &K = c->kp;
    if (K.cap_lines >= cap_lines && K.cap_tiles >= n_tiles) return 0;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    K.allocs.clear();
    K.cap_lines = std::max(cap_lines, K.cap_lines);
    K.cap_tiles = std::max(n_tiles, K.cap_tiles);
    const size_t n = (size_t)K.cap_lines + 256, nt = (size_t)std::max<int64_t>(K.cap_tiles, (K.cap_lines + 255) / 256) + 1;
    if (K.allocs.get(&K.line_start, n + 1) || K.allocs.get(&K.pos, n) || K.allocs.get(&K.idx, n) ||
        K.allocs.get(&K.ev, n) || K.allocs.get(&K.mu, n) || K.allocs.get(&K.contig, n) ||
        K.allocs.get(&K.name_off, n) || K.allocs.get(&K.name_len, n) || K.allocs.get(&K.fl, n) ||
        K.allocs.get(&K.status, n) || K.allocs.get(&K.tile_cnt, nt) || K.allocs.get(&K.tile_off, nt))
        return -10;
    return 0;
}

static int kp_set_contigs(mc_ctx *c, const char *const *names, int32_t n) {
    KpContigs &C = c->kc;
    bool same = (int)C.names.size() == n && C.hash;
    for (int i = 0; same && i < n; ++i) same = C.names[(size_t)i] == names[i];
    if (same) return 0;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    C.allocs.clear();
    C.names.assign(names, names + n);
    int size = 16;
    while (size < 2 * n + 2) size *= 2;
    std::vector<uint32_t> hash((size_t)size, 0), off((size_t)std::max(n, 1)), len((size_t)std::max(n, 1));
    std::vector<int32_t> id((size_t)size, -1);
    std::string chars;
    for (int i = 0; i < n; ++i) {
        off[(size_t)i] = (uint32_t)chars.size();
        len[(size_t)i] = (uint32_t)C.names[(size_t)i].size();
        chars += C.names[(size_t)i];
        uint32_t h = 2166136261u;
        for (unsigned char ch : C.names[(size_t)i]) h = (h ^ ch) * 16777619u;
        if (h == 0) h = 1;
        bool dup = false;                                   // the first id of a name wins, like the FASTA scan (:77-81)
        int slot = (int)(h & (uint32_t)(size - 1));
        for (; hash[(size_t)slot]; slot = (slot + 1) & (size - 1))
            if (hash[(size_t)slot] == h && C.names[(size_t)id[(size_t)slot]] == C.names[(size_t)i]) { dup = true; break; }
        if (!dup) { hash[(size_t)slot] = h; id[(size_t)slot] = i; }
    }
    chars.push_back('\0');
    C.table_mask = size - 1;
    C.n = n;
    hipStream_t us = c->up_stream;
    if (C.allocs.get(&C.hash, (size_t)size) || C.allocs.get(&C.id, (size_t)size) ||
        C.allocs.get(&C.name_off, off.size()) || C.allocs.get(&C.name_len, len.size()) ||
        C.allocs.get(&C.chars, chars.size()))
        return -10;
    HIP_TRY(hipMemcpyAsync(C.hash, hash.data(), (size_t)size * 4, hipMemcpyHostToDevice, us));
    HIP_TRY(hipMemcpyAsync(C.id, id.data(), (size_t)size * 4, hipMemcpyHostToDevice, us));
    HIP_TRY(hipMemcpyAsync(C.name_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, us));
    HIP_TRY(hipMemcpyAsync(C.name_len, len.data(), len.size() * 4, hipMemcpyHostToDevice, us));
    HIP_TRY(hipMemcpyAsync(C.chars, chars.data(), chars.size(), hipMemcpyHostToDevice, us));
    HIP_TRY(hipStreamSynchronize(us));                      // (the vectors go out of scope)
    return 0;
}

static int kp_ensure_slot(mc_ctx *c, TableSlot &S, int64_t n_bytes) {
    if (!S.ev_parsed) { if (S.ev_parsed.create() || S.ev_text_up.create()) return -10; }
    const int cap_segs = (int)std::min<int64_t>(S.cap_segs, 1 << 24);
    if (S.text && S.cap_text >= n_bytes + 64 && S.kp_cap_flags >= S.cap_rows && S.kp_cap_segs >= cap_segs) return 0;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    slot_free_parser(S);
    S.cap_text = std::max<int64_t>(n_bytes + n_bytes / 8, (int64_t)1 << 20) + 64;
    if (S.kp_allocs.get(&S.text, (size_t)S.cap_text) || S.kp_allocs.get(&S.kp_head, 1) ||
        S.kp_allocs.get(&S.kp_segs, (size_t)cap_segs) || S.kp_allocs.get(&S.kp_unknown, (size_t)KP_MAX_UNKNOWN))
        return -10;
    S.kp_cap_segs = cap_segs;
    S.kp_cap_flags = S.cap_rows;
    if (S.kp_head_h.alloc(sizeof(KpHead)) || S.kp_segs_h.alloc((size_t)cap_segs * sizeof(KpSeg)) ||
        S.kp_unknown_h.alloc((size_t)KP_MAX_UNKNOWN * sizeof(KpUnknown)) || S.kp_flags_h.alloc((size_t)S.cap_rows))
        return -10;
    return 0;
}

extern "C" int mc_ctx_parse_begin(mc_ctx *c, const char *text, int64_t n_bytes, const char *const *contig_names, int32_t n_contigs,
                                  int64_t max_rows, int32_t *slot_out) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot_out) *slot_out = -1;
    if (!text || n_bytes < 0 || n_bytes >= ((int64_t)1 << 32) || n_contigs < 0 || max_rows < 0) {
        mc_set_error("mc_ctx_parse_begin: bad arguments (%lld bytes of text; at most 4 GB per shard)", (long long)n_bytes);
        return -12;
    }
    const int at = free_slot(c, "mc_ctx_parse_begin");
    if (at < 0) return MC_E_NO_FREE_SLOT;
    TableSlot &S = c->slots[at];
    // rows: what the caller expects (the slots were sized by mc_ctx_reserve_tables, or grow here); a shard with more rows or
    // segments than the slot holds comes back from mc_ctx_parse_end as "needs the host parser"
    const int64_t rows = std::max<int64_t>(max_rows, 1);
    if (int rc = slot_ensure(c, S, rows, std::max<int64_t>(rows / 16, 64), std::max<int64_t>(rows / 16, 64))) return rc;
    if (int rc = kp_ensure_slot(c, S, n_bytes)) return rc;
    const int64_t n_tiles = (n_bytes + KP_TILE - 1) / KP_TILE;
    if (int rc = kp_ensure_scratch(c, S.cap_rows + 65536, n_tiles)) return rc;
    if (int rc = kp_set_contigs(c, contig_names, n_contigs)) return rc;
    KpScratch &K = c->kp;
    if (!c->parse_stream) { if (int rc = c->parse_stream.create()) return rc; }
    {   // the text on the upload stream, the kernels behind it on their own: the next shard's text travels while they run
        hipStream_t up = c->up_stream;
        HIP_TRY(hipStreamWaitEvent(up, S.ev_valid, 0));    // the small arrays of the slot's previous table (it may never have been scanned)
        HIP_TRY(hipEventRecord(S.ev_up_start, up));
        static const KpHead zero_head = {0, 0, 0, 0, 0, 0x7fffffffffffffffll, 0, 0};
        HIP_TRY(hipMemcpyAsync(S.kp_head, &zero_head, sizeof(KpHead), hipMemcpyHostToDevice, up));
        if (n_bytes > 0) HIP_TRY(hipMemcpyAsync(S.text, text, (size_t)n_bytes, hipMemcpyHostToDevice, up));
        HIP_TRY(hipEventRecord(S.ev_text_up, up));
    }
    hipStream_t us = c->parse_stream;
    const int kp_debug = getenv("MCALLER_KP_SYNC") ? atoi(getenv("MCALLER_KP_SYNC")) : 0;     // (finding the kernel that faults: bit i = wait behind step i)
    int kp_step = 0;
#define KP_STEP(name) do { if ((kp_debug >> kp_step++) & 1) { HIP_TRY(hipStreamSynchronize(us)); fprintf(stderr, "kp: %s ok\n", name); } } while (0)
    HIP_TRY(hipStreamWaitEvent(us, S.ev_text_up, 0));
    if (n_tiles > 0) {
        hipLaunchKernelGGL(kp_count, dim3((unsigned)n_tiles), dim3(KP_THREADS), 0, us, (const char *)S.text, n_bytes, K.tile_cnt);
        KP_STEP("kp_count");
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, us, (const long long *)K.tile_cnt, n_tiles, K.tile_off, &S.kp_head->n_newlines);
        KP_STEP("kp_scan");
        hipLaunchKernelGGL(kp_starts, dim3((unsigned)n_tiles), dim3(KP_THREADS), 0, us, (const char *)S.text, n_bytes,
                           (const long long *)K.tile_off, K.line_start, K.cap_lines, S.kp_head);
        KP_STEP("kp_starts");
        const int64_t cap_lines = K.cap_lines;
        const unsigned line_blocks = (unsigned)((cap_lines + 255) / 256);
        KpParseArgs PA;
        PA.text = S.text; PA.n_bytes = n_bytes; PA.line_start = K.line_start; PA.head = S.kp_head; PA.head_w = S.kp_head;
        PA.cap_lines = cap_lines; PA.c_hash = c->kc.hash; PA.c_id = c->kc.id; PA.c_off = c->kc.name_off; PA.c_len = c->kc.name_len;
        PA.c_chars = c->kc.chars; PA.c_mask = c->kc.table_mask;
        PA.pos = K.pos; PA.idx = K.idx; PA.ev = K.ev; PA.mu = K.mu; PA.contig = K.contig; PA.name_off = K.name_off; PA.name_len = K.name_len;
        PA.fl = K.fl; PA.status = K.status;
        hipLaunchKernelGGL(kp_parse, dim3(line_blocks), dim3(256), KP_STAGE + 16, us, PA);
        KP_STEP("kp_parse");
        hipLaunchKernelGGL(kp_count_rows, dim3(line_blocks), dim3(256), 0, us, (const uint8_t *)K.status, (const KpHead *)S.kp_head,
                           cap_lines, K.tile_cnt);
        KP_STEP("kp_count_rows");
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, us, (const long long *)K.tile_cnt, (int64_t)line_blocks, K.tile_off,
                           &S.kp_head->n_rows);
        KP_STEP("kp_scan");
        KpPlaceArgs QA;
        QA.text = S.text; QA.head = S.kp_head; QA.head_w = S.kp_head; QA.cap_lines = cap_lines; QA.cap_rows = S.cap_rows;
        QA.blk_off = K.tile_off; QA.pos = K.pos; QA.idx = K.idx; QA.ev = K.ev; QA.mu = K.mu; QA.contig = K.contig;
        QA.name_off = K.name_off; QA.name_len = K.name_len; QA.fl = K.fl; QA.status = K.status;
        QA.t_pos = S.pos; QA.t_idx = S.idx; QA.t_evmu = S.evmu; QA.t_flags = S.flags; QA.t_nbits = S.nbits; QA.t_xrel = S.xrel; QA.t_prel = S.prel; QA.t_unit_pp = S.unit_pp; QA.segs = S.kp_segs; QA.cap_segs = S.kp_cap_segs;
        QA.unknown = S.kp_unknown;
        hipLaunchKernelGGL(kp_place, dim3(line_blocks), dim3(256), 0, us, QA);
        KP_STEP("kp_place");
    }
    // what mc_ctx_parse_end hands out, on its way as soon as it exists: the head, the first segments and unknown tokens (a
    // shard with more of them gets the rest when it is waited for), the flag column
    // (by kernel: a DMA transfer would queue behind the text of the shards that follow)
    S.kp_flags_sent = std::min<int64_t>(S.cap_rows, std::min<int64_t>(rows + rows / 4 + 4096, (int64_t)COPY_BY_KERNEL_MAX));
    if (int rc = mc_copy_by_kernel(S.kp_segs_h.p, S.kp_segs, (size_t)std::min(S.kp_cap_segs, KP_EAGER_SEGS) * sizeof(KpSeg), us)) return rc;
    if (int rc = mc_copy_by_kernel(S.kp_unknown_h.p, S.kp_unknown, (size_t)KP_EAGER_UNKNOWN * sizeof(KpUnknown), us)) return rc;
    if (int rc = mc_copy_by_kernel(S.kp_flags_h.p, S.flags, (size_t)S.kp_flags_sent, us)) return rc;
    if (int rc = mc_copy_by_kernel(S.kp_head_h.p, S.kp_head, sizeof(KpHead), us)) return rc;
    HIP_TRY(hipEventRecord(S.ev_parsed, us));
    KP_STEP("copies");
#undef KP_STEP
    HIP_TRY(hipGetLastError());
    S.refs += 1;                                            // the slot is taken until mc_ctx_parse_finish / _abandon
    S.holds_table = false;                                  // (the columns are being overwritten: S.T describes them no more)
    S.from_parser = false;
    S.kp_state = 1;
    if (slot_out) *slot_out = at;
    return 0;
}

static int kp_slot(mc_ctx *c, int32_t slot, int state, const char *who, TableSlot **S) {
    if (slot < 0 || slot >= MC_TABLE_SLOTS || c->slots[slot].kp_state != state) {
        mc_set_error("%s: slot %d is not in that state", who, slot);
        return -12;
    }
    *S = &c->slots[slot];
    return 0;
}

extern "C" int mc_ctx_parse_end(mc_ctx *c, int32_t slot, mc_devparse_result *out) {
    HIP_TRY(hipSetDevice(c->device));
    TableSlot *Sp;
    if (int rc = kp_slot(c, slot, 1, "mc_ctx_parse_end", &Sp)) return rc;
    TableSlot &S = *Sp;
    memset(out, 0, sizeof(*out));
    HIP_TRY(hipEventSynchronize(S.ev_parsed));
    const KpHead H = *S.kp_head_h.get<KpHead>();
    S.kp_state = 2;
    out->n_lines = H.n_lines; out->n_rows = H.n_rows; out->n_seg = H.n_seg; out->n_unknown = H.n_unknown;
    if (H.overflow || H.first_host_line != 0x7fffffffffffffffll || H.n_rows > S.cap_rows || H.n_seg > S.kp_cap_segs) {
        out->status = 1;
        if (H.first_host_line != 0x7fffffffffffffffll)
            mc_set_error("device parser: line %lld needs the host parser (a number form or value beyond the fast path)", H.first_host_line);
        else
            mc_set_error("device parser: %lld lines, %lld rows, %d segments, %d unknown-contig lines do not fit the slot", H.n_lines, H.n_rows,
                         H.n_seg, H.n_unknown);
        return 0;
    }
    // (what did not travel with the head: blocking copies -- the streams are busy with the next shard)
    KpSeg *segs_h = S.kp_segs_h.get<KpSeg>();
    KpUnknown *unknown_h = S.kp_unknown_h.get<KpUnknown>();
    if (H.n_seg > KP_EAGER_SEGS) HIP_TRY(hipMemcpy(segs_h, S.kp_segs, (size_t)H.n_seg * sizeof(KpSeg), hipMemcpyDeviceToHost));
    if (H.n_unknown > KP_EAGER_UNKNOWN) HIP_TRY(hipMemcpy(unknown_h, S.kp_unknown, (size_t)H.n_unknown * sizeof(KpUnknown), hipMemcpyDeviceToHost));
    if (H.n_rows > S.kp_flags_sent) HIP_TRY(hipMemcpy(S.kp_flags_h.p, S.flags, (size_t)H.n_rows, hipMemcpyDeviceToHost));
    // segments and unknown lines were listed in the order the lanes got there: file order is by row / by line
    std::sort(segs_h, segs_h + H.n_seg, [](const KpSeg &a, const KpSeg &b) { return a.row < b.row; });
    std::sort(unknown_h, unknown_h + H.n_unknown, [](const KpUnknown &a, const KpUnknown &b) { return a.line < b.line; });
    S.kp_seg_row.resize((size_t)H.n_seg); S.kp_seg_off.resize((size_t)H.n_seg); S.kp_seg_contig.resize((size_t)H.n_seg);
    S.kp_seg_len.resize((size_t)H.n_seg); S.kp_seg_ns.resize((size_t)H.n_seg);
    for (int i = 0; i < H.n_seg; ++i) {
        const KpSeg &g = segs_h[i];
        S.kp_seg_row[(size_t)i] = g.row; S.kp_seg_off[(size_t)i] = g.name_off; S.kp_seg_contig[(size_t)i] = g.contig;
        S.kp_seg_len[(size_t)i] = g.name_len; S.kp_seg_ns[(size_t)i] = (uint8_t)g.name_start;
    }
    S.kp_unk_off.resize((size_t)H.n_unknown); S.kp_unk_len.resize((size_t)H.n_unknown);
    for (int i = 0; i < H.n_unknown; ++i) { S.kp_unk_off[(size_t)i] = unknown_h[i].off; S.kp_unk_len[(size_t)i] = unknown_h[i].len; }
    out->seg_row_begin = S.kp_seg_row.data(); out->seg_contig = S.kp_seg_contig.data(); out->seg_name_off = S.kp_seg_off.data();
    out->seg_name_len = S.kp_seg_len.data(); out->seg_name_start = S.kp_seg_ns.data();
    out->unknown_off = S.kp_unk_off.data(); out->unknown_len = S.kp_unk_len.data();
    out->flags = S.kp_flags_h.get<uint8_t>();
    return 0;
}

extern "C" int mc_ctx_parse_finish(mc_ctx *c, int32_t slot, const int32_t *seg_read, int32_t n_reads, const double *read_qual) {
    HIP_TRY(hipSetDevice(c->device));
    TableSlot *Sp;
    if (int rc = kp_slot(c, slot, 2, "mc_ctx_parse_finish", &Sp)) return rc;
    TableSlot &S = *Sp;
    const KpHead H = *S.kp_head_h.get<KpHead>();
    if (H.n_seg > S.cap_segs || n_reads > S.cap_reads) {
        // (the small arrays of the slot were sized for fewer segments / reads: grow them; the columns stay)
        mc_set_error("mc_ctx_parse_finish: %d segments, %d reads: the slot holds %lld, %lld (mc_ctx_reserve_tables)", H.n_seg, n_reads,
                     (long long)S.cap_segs, (long long)S.cap_reads);
        return -12;
    }
    HIP_TRY(hipEventSynchronize(S.ev_uploaded));           // the stage is about to be rewritten (long done: the slot was idle)
    S.kp_state = 0;
    S.refs = std::max(S.refs - 1, 0);
    if (int rc = fill_slot(c, slot, H.n_rows, H.n_seg, S.kp_seg_row.data(), seg_read, S.kp_seg_contig.data(), S.kp_seg_ns.data(), n_reads,
                           read_qual, nullptr))
        return rc;
    return 0;
}

extern "C" int mc_ctx_parse_abandon(mc_ctx *c, int32_t slot) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || c->slots[slot].kp_state == 0) {
        mc_set_error("mc_ctx_parse_abandon: slot %d holds no parse", slot);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipEventSynchronize(S.ev_parsed));
    // (ev_valid still stands for the slot's previous table, which is all a later upload waits for)
    S.kp_state = 0;
    S.refs = std::max(S.refs - 1, 0);
    return 0;
}

// the columns of a slot's table back on the host (tests: the device parser's columns against the host parser's)
extern "C" int mc_ctx_fetch_columns(mc_ctx *c, int32_t slot, int64_t n_rows, int32_t *pos, int32_t *event_model_e4, int32_t *event_idx,
                                    uint8_t *flags) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].pos || n_rows < 0 || n_rows > c->slots[slot].cap_rows) {
        mc_set_error("mc_ctx_fetch_columns: slot %d, %lld rows", slot, (long long)n_rows);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    if (n_rows == 0) return 0;
    if (pos) HIP_TRY(hipMemcpy(pos, S.pos, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
    if (event_model_e4) HIP_TRY(hipMemcpy(event_model_e4, S.evmu, (size_t)n_rows * 8, hipMemcpyDeviceToHost));
    if (event_idx) HIP_TRY(hipMemcpy(event_idx, S.idx, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, S.flags, (size_t)n_rows, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mc_ctx_fetch_model_n_bits(mc_ctx *c, int32_t slot, int64_t n_rows, uint8_t *out) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].pos || n_rows < 0 || n_rows > c->slots[slot].cap_rows || !out) {
        mc_set_error("mc_ctx_fetch_model_n_bits: slot %d, %lld rows", slot, (long long)n_rows);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    if (n_rows > 0) HIP_TRY(hipMemcpy(out, S.nbits, (size_t)(n_rows + 7) / 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mc_ctx_fetch_idx_rel_bits(mc_ctx *c, int32_t slot, int64_t n_rows, uint16_t *out) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].pos || n_rows < 0 || n_rows > c->slots[slot].cap_rows || !out) {
        mc_set_error("mc_ctx_fetch_idx_rel_bits: slot %d, %lld rows", slot, (long long)n_rows);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    if (n_rows > 0) HIP_TRY(hipMemcpy(out, S.xrel, (size_t)(n_rows + 7) / 8 * 2, hipMemcpyDeviceToHost));
    return 0;
}

// ... its position-relation column, likewise
extern "C" int mc_ctx_fetch_pos_rel_bits(mc_ctx *c, int32_t slot, int64_t n_rows, uint16_t *out) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].pos || n_rows < 0 || n_rows > c->slots[slot].cap_rows || !out) {
        mc_set_error("mc_ctx_fetch_pos_rel_bits: slot %d, %lld rows", slot, (long long)n_rows);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    if (n_rows > 0) HIP_TRY(hipMemcpy(out, S.prel, (size_t)(n_rows + 7) / 8 * 2, hipMemcpyDeviceToHost));
    return 0;
}

// ... and its unit summaries: ceil(n_rows / 8) pairs (first, last position of the unit; the second of a last, partial unit is
// whatever the slot holds there)
extern "C" int mc_ctx_fetch_unit_summaries(mc_ctx *c, int32_t slot, int64_t n_rows, int32_t *out) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].pos || n_rows < 0 || n_rows > c->slots[slot].cap_rows || !out) {
        mc_set_error("mc_ctx_fetch_unit_summaries: slot %d, %lld rows", slot, (long long)n_rows);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    if (c->parse_stream) HIP_TRY(hipStreamSynchronize(c->parse_stream));
    if (n_rows > 0) HIP_TRY(hipMemcpy(out, S.unit_pp, (size_t)(n_rows + 7) / 8 * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mc_ctx_wait_upload(mc_ctx *c, int32_t slot) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].ev_uploaded) {
        mc_set_error("mc_ctx_wait_upload: slot %d", slot);
        return -12;
    }
    HIP_TRY(hipEventSynchronize(c->slots[slot].ev_uploaded));
    return 0;
}

extern "C" int mc_ctx_current_slot(mc_ctx *c) { return c->cur; }

// A resident table becomes the current one again (the passes enqueued afterwards scan it).  as_new != 0: what earlier passes
// left behind for later ones is set aside -- the next pass does everything the first pass over a table does (classification on
// the blocks' first rows, positions and event indices streamed, every row validated).
extern "C" int mc_ctx_select_table(mc_ctx *c, int32_t slot, int32_t as_new) {
    HIP_TRY(hipSetDevice(c->device));
    // (holds_table: set when a table's small arrays went in, fill_slot; cleared when a parse began to overwrite the columns -- a
    // parse that was abandoned, or handed out and never finished, leaves columns that S.T does not describe)
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].T.pos || c->slots[slot].kp_state != 0 || !c->slots[slot].holds_table) {
        mc_set_error("mc_ctx_select_table: slot %d holds no complete table", slot);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    c->T = S.T;
    c->cur = slot;
    if (S.qual) { c->qual = S.qual; c->n_qual = S.n_qual; }
    else { c->qual = c->qual_own; c->n_qual = c->n_qual_own; }
    // (passes over the slot that are still in flight keep the plan they were enqueued with; a first pass only ORs what it sees
    // into the table's validation flags, so declaring the table new beside them is safe as long as they are first passes too --
    // bench.py's steps -- and a caller that mixes pass kinds waits for them first)
    if (as_new) {
        S.passes = 0;
        S.tmpl_ref = -1;          // (the name-block templates too: they are part of what a table costs when it is scanned once)
    }
    return 0;
}

extern "C" int mc_ctx_upload_times_ms(mc_ctx *c, int32_t slot, float *h2d_ms, float *validate_ms) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || !c->slots[slot].ev_uploaded) {
        mc_set_error("mc_ctx_upload_times_ms: slot %d", slot);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipEventSynchronize(S.ev_valid));
    if (h2d_ms) HIP_TRY(hipEventElapsedTime(h2d_ms, S.ev_up_start, S.ev_uploaded));
    if (validate_ms) HIP_TRY(hipEventElapsedTime(validate_ms, S.ev_val_start, S.ev_valid));
    return 0;
}

extern "C" int mc_ctx_parse_times_ms(mc_ctx *c, int32_t slot, float *text_h2d_ms, float *parse_ms) {
    HIP_TRY(hipSetDevice(c->device));
    if (slot < 0 || slot >= MC_TABLE_SLOTS || c->slots[slot].kp_state == 0 || !c->slots[slot].ev_parsed) {
        mc_set_error("mc_ctx_parse_times_ms: slot %d holds no parse", slot);
        return -12;
    }
    TableSlot &S = c->slots[slot];
    HIP_TRY(hipEventSynchronize(S.ev_parsed));
    if (text_h2d_ms) HIP_TRY(hipEventElapsedTime(text_h2d_ms, S.ev_up_start, S.ev_text_up));
    if (parse_ms) HIP_TRY(hipEventElapsedTime(parse_ms, S.ev_text_up, S.ev_parsed));
    return 0;
}

extern "C" int mc_ctx_upload_table(mc_ctx *c, const mc_table_view *h) {
    HIP_TRY(hipSetDevice(c->device));
    // the one-table interface: whatever is in flight finishes first, so the caller's buffers are free on return and the
    // slot that is taken over holds nothing anybody waits for
    if (int rc = mc_sync_pass_streams(c)) return rc;
    if (c->ab_count == 0) {                                  // no pass to hand out any more: nothing is held
        c->held = -1;
        for (TableSlot &S : c->slots) S.refs = S.kp_state != 0 ? 1 : 0;      // (but a slot the device parser is filling stays taken)
    }
    int32_t slot = -1;
    if (int rc = mc_ctx_upload_table_async(c, h, nullptr, &slot)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
