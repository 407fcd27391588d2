// mc_xmfamap.inc -- two genomes with their own assemblies compared through a Mauve alignment: the XMFA text into a coordinate map
// on the GPU, and bed1's lines lifted through it onto bed2's keys.  Part of the mc_bedcompare.hip unit (included there, inside its
// unnamed namespace, behind kc_probe): kc_lift stands in kc_probe's place and everything from kc_sites on runs as it is.  The
// definition -- lines, entries, columns, first-wins, the lift -- stands in mcaller_amd/compare_genomes.py; C ABI: mc_xmfa_map,
// mc_xmfa_map_last_stats, mc_xmfa_map_release, mc_bed_compare with its contig tables; Python: Device.xmfa_map,
// Device.bed_compare(contigs1=, contigs2=), compare_genomes.compare_by_position_device(xmfa_path=).
//
// The map is map[g1] = (the column's ordinal among the paired columns of the file) << 33 | g2 << 1 | flip, ~0: unmapped, 8 bytes a
// base of genome 1, resident in the context (mc_ctx::xmfa_map) from mc_xmfa_map to the next such call or mc_xmfa_map_release.
// Declines (status 1, mc_last_error, mc_xmfa_map_last_stats: reason and line; no map is kept):
//   line by line   MC_CMP_DECLINE_XMFA_BYTE      a '\r' or a byte >= 0x80, on any line (comments too)
//                  MC_CMP_DECLINE_XMFA_HEADER    a header that is not `>[blanks]SEQ:START-END blanks +|- [blank anything]` with START-END
//                                                0-0 or 1 <= START <= END (numbers beyond 2^40 count as malformed here; the host
//                                                words them), or a sequence line before its block's first header
//                  MC_CMP_DECLINE_XMFA_SEQ_BYTE  a sequence byte that is neither '-' nor a letter
//   entry by entry (a file whose lines are sound; the header's line is named)
//                  MC_CMP_DECLINE_XMFA_COUNT     non-gaps other than END - START + 1 (0 for 0-0)
//                  MC_CMP_DECLINE_XMFA_COLUMNS   another column count than the entry before it in the block
//                  MC_CMP_DECLINE_XMFA_UNCLOSED  an entry behind the last '='
//                  MC_CMP_DECLINE_XMFA_RANGE     an END beyond n1 (entries of seq1) or n2 (of seq2)
//   file-level     MC_CMP_DECLINE_XMFA_GENOME    n1 or n2 over 2^31 - 2, or 2^31 paired columns or more (the map's word holds 31 bits
//                                                of ordinal and 32 of g2)
//                  MC_CMP_DECLINE_ROWS           2^31 - 2 lines or more
//                  MC_CMP_DECLINE_MEMORY         the text, its tables and the map beside free device memory (MCALLER_CMP_DEVICE_BYTES)
//   the lift       MC_CMP_DECLINE_LIFT_START     a bed1 start that is not plain digits: int() may accept it, the host decides
// Of several offending lines the first is named, of several reasons on it the smallest (line_flag).
//
// The steps (L lines, E entries, B blocks, C columns of the paired blocks, W = their 64-column words):
//   kp_count / kp_scan / kp_starts   line starts (mc_lines.h, launched by mc_textfeed.h)
//   kx_lines     a lane per line: comment, blank, header, '=' or sequence; ByteClass and '\r'; a header's four fields in integers;
//                a sequence line's length and non-gap count
//   kp_scan x 4  headers before a line (its entry), '=' before it (its block), columns and non-gaps before it
//   kx_place     a lane per line: an entry's header line, the entries in front of each '='
//   kx_check     a lane per line: a sequence line whose block has no header yet
//   kx_entries   a lane per entry: columns and non-gaps (differences of the scans) against the header and the entry before it; the
//                block's first entry of seq1 and of seq2 by integer atomicMin
//   kx_blocks    a lane per block: paired or not, its columns, words and the two headers' fields; kp_scan x 2: where a block's
//                columns and words begin (words are block-aligned)
//   kx_pack      a lane per sequence line of a paired entry: its non-gap flags into the entry's bit-plane, 64 columns a word, by
//                integer atomicOr (a line ends where it ends: most words are shared by two lines); kx_popc + kp_scan x 2: the
//                non-gaps in front of each word
//   kx_columns   THE HOT PATH, a lane per column of the paired blocks: the block by binary search in the blocks' first columns,
//                the two bits, each rank = the word's prefix less the block's + popcount of the bits below, g1, g2, flip, one
//                64-bit integer atomicMin into map[g1]: the first column in file order wins whatever order the lanes arrive in
//   kx_view      at most 2048 workgroups stride over the bases: the mapped ones counted (a sum a workgroup, one integer atomicAdd
//                each: a lane per base with an atomicAdd a wave took 0.87 ms at 4.6 * 10^6 bases, all on one address), g2 and
//                flip unpacked for the view
//   kc_contigs   a lane per contig of genome 1: its name into a key table (kt_claim; of two contigs with one name the first stays)
//   kc_lift      a lane per bed1 line, behind kc_parse and bed2's kc_insert: chrom -> kt_find -> g1 -> map -> the contig of g2 by
//                binary search in genome 2's offsets; the image key is never written out: its digits (mc_rowtext.h: rt_put_uint) go
//                straight into KeyHash, pieces and separators as kc_parse hashes a key, and into the byte comparison against the
//                probed slot's bed2 line.  kc_size / kc_write copy the image's four fields from that line
// No floating point; no atomic decides an order of output.
// A sequence line is walked by one lane in kx_lines and in kx_pack: a file whose sequences are not wrapped (lines of megabytes) is
// read correctly and slowly.
// Resources (tools/kres.py, gfx950; no kernel spills or uses scratch; kx_view has 16 bytes of LDS, the others none):
//   VGPRs: kx_lines 25, kx_place 8, kx_check 8, kx_entries 36, kx_blocks 24, kx_pack 18, kx_popc 10, kx_columns 28, kx_view 14,
//   kc_contigs 21, kc_lift 56 -- 8 waves a SIMD every one of them

constexpr int XK_BLANK = 0, XK_COMMENT = 1, XK_HEADER = 2, XK_END = 3, XK_SEQ = 4;
constexpr long long XM_COORD_CAP = (1ll << 31) - 2;
constexpr unsigned long long XM_UNMAPPED = ~0ull;

struct XmBlock {                             // a paired block: the two entries' header fields
    long long s1, e1, s2, e2;
    int minus1, minus2;
};

struct XmHead {
    KpHead kp;
    unsigned long long decline;
    long long n_entries, n_blocks, n_cols_all, n_nongap_all;      // totals of the line scans
    long long n_pcols, n_words, n_rank1, n_rank2;                 // totals of the block and word scans
    unsigned long long n_paired, n_mapped;
};

struct XmArgs {
    const char *text;
    int64_t n_bytes, n_nl;
    const long long *line_start;
    XmHead *head;
    int64_t seq1, seq2, n1, n2;
    // per line
    uint8_t *kind, *h_minus;
    long long *is_hdr, *is_end, *cols, *nongap;      // what the scans take
    long long *ent_of, *blk_of, *col_off, *ng_off;   // headers, '=', columns, non-gaps in front of the line
    long long *h_seq, *h_start, *h_end;
    // per entry (E + 1: the line count behind the last) and per block
    int64_t E, B;
    long long *hl, *ent_cols, *blk_ent_end;
    int *blk_e1, *blk_e2;
    long long *pcols, *pwords, *pcol_off, *pword_off;
    XmBlock *blocks;
    // the gap planes and the map
    int64_t W, C;
    unsigned long long *plane1, *plane2;
    long long *cnt1, *cnt2, *pre1, *pre2;
    unsigned long long *map;
    long long *view_g2;
    uint8_t *view_flip;
};

__device__ __forceinline__ bool xm_blank(char c) { return c == ' ' || c == '\t'; }

// digits at t[*i ...) -> their value (one beyond 2^40 stays beyond it), *i behind them; false: no digit
__device__ __forceinline__ bool xm_number(const char *t, int64_t len, int64_t *i, long long *v) {
    long long a = 0;
    const int64_t i0 = *i;
    while (*i < len && (unsigned)(t[*i] - '0') < 10u) {
        a = a > (1ll << 40) ? a : a * 10 + (t[*i] - '0');
        ++*i;
    }
    *v = a;
    return *i > i0;
}

__device__ __forceinline__ bool xm_header(const char *t, int64_t len, long long *seq, long long *start, long long *end, int *minus) {
    int64_t i = 1;
    while (i < len && xm_blank(t[i])) ++i;
    if (!xm_number(t, len, &i, seq) || i >= len || t[i] != ':') return false;
    ++i;
    if (!xm_number(t, len, &i, start) || i >= len || t[i] != '-') return false;
    ++i;
    if (!xm_number(t, len, &i, end)) return false;
    const int64_t i0 = i;
    while (i < len && xm_blank(t[i])) ++i;
    if (i == i0 || i >= len || (t[i] != '+' && t[i] != '-')) return false;
    *minus = t[i] == '-';
    ++i;
    if (i < len && !xm_blank(t[i])) return false;
    if (*seq > (1ll << 40) || *start > (1ll << 40) || *end > (1ll << 40)) return false;
    return (*start == 0 && *end == 0) || (1 <= *start && *start <= *end);
}

__global__ __launch_bounds__(256) void kx_lines(XmArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.head->kp.n_lines) return;
    const int64_t b = A.line_start[li];
    const int64_t e = li < A.n_nl ? (int64_t)A.line_start[li + 1] - 1 : A.n_bytes;
    const char *t = A.text + b;
    const int64_t len = e - b;
    const char c0 = len > 0 ? t[0] : '\0';
    const int kind = len == 0 ? XK_BLANK : c0 == '#' ? XK_COMMENT : (c0 == '=' && len == 1) ? XK_END : c0 == '>' ? XK_HEADER : XK_SEQ;
    ByteClass bad;
    bool cr = false, not_seq = false;
    long long letters = 0;
    for (int64_t i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)t[i];
        bad.see(c);
        cr |= c == '\r';
        const bool letter = ((c | 0x20u) - 'a') < 26u;
        not_seq |= !(letter || c == '-');
        letters += letter ? 1 : 0;
    }
    long long seq = 0, start = 0, end = 0;
    int minus = 0;
    if (bad.hi || cr) line_flag(&A.head->decline, li, MC_CMP_DECLINE_XMFA_BYTE);
    else if (kind == XK_HEADER && !xm_header(t, len, &seq, &start, &end, &minus)) line_flag(&A.head->decline, li, MC_CMP_DECLINE_XMFA_HEADER);
    else if (kind == XK_SEQ && not_seq) line_flag(&A.head->decline, li, MC_CMP_DECLINE_XMFA_SEQ_BYTE);
    A.kind[li] = (uint8_t)kind;
    A.is_hdr[li] = kind == XK_HEADER; A.is_end[li] = kind == XK_END;
    A.cols[li] = kind == XK_SEQ ? len : 0; A.nongap[li] = kind == XK_SEQ ? letters : 0;
    A.h_seq[li] = seq; A.h_start[li] = start; A.h_end[li] = end; A.h_minus[li] = (uint8_t)minus;
}

__global__ __launch_bounds__(256) void kx_place(XmArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t L = A.head->kp.n_lines;
    if (li == 0) A.hl[A.head->n_entries] = L;
    if (li >= L) return;
    if (A.kind[li] == XK_HEADER) A.hl[A.ent_of[li]] = li;
    if (A.kind[li] == XK_END) A.blk_ent_end[A.blk_of[li]] = A.ent_of[li];
}

__global__ __launch_bounds__(256) void kx_check(XmArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.head->kp.n_lines || A.kind[li] != XK_SEQ) return;
    const long long k = A.blk_of[li];
    if (A.ent_of[li] == (k > 0 ? A.blk_ent_end[k - 1] : 0)) line_flag(&A.head->decline, li, MC_CMP_DECLINE_XMFA_HEADER);
}

// a scan's value in front of line i, the total behind the last line
__device__ __forceinline__ long long xm_before(const long long *off, int64_t i, int64_t n, long long total) { return i < n ? off[i] : total; }

__global__ __launch_bounds__(256) void kx_entries(XmArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= A.E) return;
    const int64_t L = A.head->kp.n_lines;
    const long long line = A.hl[e], next = A.hl[e + 1];
    const long long cols = xm_before(A.col_off, next, L, A.head->n_cols_all) - A.col_off[line];
    const long long letters = xm_before(A.ng_off, next, L, A.head->n_nongap_all) - A.ng_off[line];
    const long long seq = A.h_seq[line], start = A.h_start[line], end = A.h_end[line], k = A.blk_of[line];
    A.ent_cols[e] = cols;
    const bool closed = k < A.head->n_blocks;
    if (letters != (end == 0 ? 0 : end - start + 1)) line_flag(&A.head->decline, line, MC_CMP_DECLINE_XMFA_COUNT);
    else if (e > 0 && A.blk_of[A.hl[e - 1]] == k && A.col_off[line] - A.col_off[A.hl[e - 1]] != cols)
        line_flag(&A.head->decline, line, MC_CMP_DECLINE_XMFA_COLUMNS);
    else if (!closed) line_flag(&A.head->decline, line, MC_CMP_DECLINE_XMFA_UNCLOSED);
    else if ((seq == A.seq1 && end > A.n1) || (seq == A.seq2 && end > A.n2)) line_flag(&A.head->decline, line, MC_CMP_DECLINE_XMFA_RANGE);
    if (closed && seq == A.seq1) atomicMin(&A.blk_e1[k], (int)e);
    if (closed && seq == A.seq2) atomicMin(&A.blk_e2[k], (int)e);
}

__global__ __launch_bounds__(256) void kx_blocks(XmArgs A) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.B) return;
    const long long e1 = A.blk_e1[k], e2 = A.blk_e2[k];
    XmBlock b = {};
    long long cols = 0;
    if (e1 < A.E && e2 < A.E) {
        const long long l1 = A.hl[e1], l2 = A.hl[e2];
        b.s1 = A.h_start[l1]; b.e1 = A.h_end[l1]; b.minus1 = A.h_minus[l1];
        b.s2 = A.h_start[l2]; b.e2 = A.h_end[l2]; b.minus2 = A.h_minus[l2];
        if (b.e1 != 0 && b.e2 != 0) cols = A.ent_cols[e1];
    }
    A.blocks[k] = b;
    A.pcols[k] = cols;
    A.pwords[k] = (cols + 63) >> 6;
    if (cols > 0) atomicAdd(&A.head->n_paired, 1ull);
}

__global__ __launch_bounds__(256) void kx_pack(XmArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.head->kp.n_lines || A.kind[li] != XK_SEQ) return;
    const long long e = A.ent_of[li] - 1, k = A.blk_of[li];
    if (e < 0 || k >= A.B || A.pcols[k] == 0) return;
    unsigned long long *plane = e == A.blk_e1[k] ? A.plane1 : e == A.blk_e2[k] ? A.plane2 : nullptr;
    if (!plane) return;
    const int64_t b = A.line_start[li];
    const int64_t len = (li < A.n_nl ? (int64_t)A.line_start[li + 1] - 1 : A.n_bytes) - b;
    const char *t = A.text + b;
    const long long c0 = A.col_off[li] - A.col_off[A.hl[e]];
    const long long w_end = A.pword_off[k] + A.pwords[k];
    long long w = A.pword_off[k] + (c0 >> 6);
    int bit = (int)(c0 & 63);
    unsigned long long acc = 0;
    for (int64_t i = 0; i < len; ++i) {
        acc |= t[i] != '-' ? 1ull << bit : 0ull;
        if (++bit == 64) {
            if (acc && w < w_end) atomicOr(&plane[w], acc);
            acc = 0; bit = 0; ++w;
        }
    }
    if (acc && w < w_end) atomicOr(&plane[w], acc);
}

__global__ __launch_bounds__(256) void kx_popc(XmArgs A) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= A.W) return;
    A.cnt1[w] = __popcll(A.plane1[w]);
    A.cnt2[w] = __popcll(A.plane2[w]);
}

__global__ __launch_bounds__(256) void kx_columns(XmArgs A) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= A.C) return;
    int64_t lo = 0, hi = A.B;                                          // the last block whose first column is at or before c
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.pcol_off[mid] <= c) lo = mid; else hi = mid;
    }
    const long long j = c - A.pcol_off[lo];
    if (j >= A.pcols[lo]) return;                                      // (cannot be: the scan counted these columns)
    const long long w0 = A.pword_off[lo], w = w0 + (j >> 6);
    const int bit = (int)(j & 63);
    const unsigned long long m1 = A.plane1[w], m2 = A.plane2[w];
    if (!((m1 >> bit) & (m2 >> bit) & 1ull)) return;
    const unsigned long long below = (1ull << bit) - 1ull;
    const long long r1 = A.pre1[w] - A.pre1[w0] + __popcll(m1 & below), r2 = A.pre2[w] - A.pre2[w0] + __popcll(m2 & below);
    const XmBlock b = A.blocks[lo];
    const long long g1 = b.minus1 ? b.e1 - r1 : b.s1 + r1, g2 = b.minus2 ? b.e2 - r2 : b.s2 + r2;
    if (g1 < 1 || g1 > A.n1 || g2 < 1 || g2 > A.n2) return;            // (cannot be: the counts and ENDs were checked)
    atomicMin(&A.map[g1], ((unsigned long long)c << 33) | ((unsigned long long)g2 << 1) | (unsigned long long)(b.minus1 != b.minus2));
}

__global__ __launch_bounds__(256) void kx_view(XmArgs A) {
    __shared__ unsigned s_w[4];
    unsigned mine = 0;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g <= A.n1; g += (int64_t)gridDim.x * 256) {
        const unsigned long long m = A.map[g];
        const bool mapped = m != XM_UNMAPPED;
        mine += mapped ? 1u : 0u;
        if (A.view_g2) {
            A.view_g2[g] = mapped ? (long long)((m >> 1) & 0xffffffffull) : 0;
            A.view_flip[g] = mapped ? (uint8_t)(m & 1ull) : (uint8_t)0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = mine;
    __syncthreads();
    const unsigned total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (threadIdx.x == 0 && total) atomicAdd(&A.head->n_mapped, (unsigned long long)total);
}

// ---- the lift ----
__device__ __forceinline__ bool xl_same_id(const LiftDev &T, const char *p, int n, int64_t r) {
    return T.id_off1[r + 1] - T.id_off1[r] == n && same_bytes(p, T.ids1 + T.id_off1[r], n);
}

__global__ __launch_bounds__(256) void kc_contigs(LiftDev T, unsigned long long *table, uint64_t hash_mask) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= T.nc1) return;
    const char *p = T.ids1 + T.id_off1[c];
    const int n = (int)(T.id_off1[c + 1] - T.id_off1[c]);
    KeyHash H;
    H.span(p, n);
    const uint64_t h = H.done(hash_mask);
    const KtHit hit = kt_claim(table, T.cmask, h, c, [&](int64_t r) { return xl_same_id(T, p, n, r); });
    if (hit.slot >= 0 && !hit.claimed) atomicMin(&table[hit.slot], kt_word(h, c));      // one name twice: the first contig stays
}

// where the digits of a number go: into a key's hash, or against the bytes of a field
struct XlHash {
    KeyHash *H;
    __device__ __forceinline__ void put(char c) { H->put(c); }
};
struct XlSame {
    const char *p;
    int n, at;
    bool ok;
    __device__ __forceinline__ void put(char c) { ok = ok && at < n && p[at] == c; ++at; }
};
__device__ __forceinline__ bool xl_same_number(const char *p, int n, uint32_t v) {
    XlSame s{p, n, 0, true};
    rt_put_uint(s, v);
    return s.ok && s.at == n;
}

__global__ __launch_bounds__(256) void kc_lift(CmpArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1) return;
    const LiftDev &T = A.lift;
    long long found = -1;
    int looked = 0;
    bool image = false;
    const TabSpan L = cmp_line(A, li);
    if (L.len != 0) {
        const char *t = A.text + A.line_start[li];
        const char *st = t + L.t[0] + 1;
        const int n_st = L.t[1] - L.t[0] - 1;
        bool plain = n_st >= 1 && n_st <= 10 && (st[0] != '0' || n_st == 1);
        long long start = 0;
        for (int i = 0; i < n_st && i < 10; ++i) {
            plain = plain && (unsigned)(st[i] - '0') < 10u;
            start = start * 10 + (st[i] - '0');
        }
        bool digits = true;                                            // (more than ten plain digits: a start past every contig)
        for (int i = 0; i < n_st; ++i) digits = digits && (unsigned)(st[i] - '0') < 10u;
        const bool too_long = digits && n_st > 10 && st[0] != '0';
        if (!plain && !too_long) line_flag(&A.head->decline, li, MC_CMP_DECLINE_LIFT_START);
        const char strand = t[L.t[4] + 1];
        const bool stranded = L.t[5] - L.t[4] == 2 && (strand == '+' || strand == '-');
        KeyHash Hc;
        Hc.span(t, L.t[0]);
        const KtHit contig = kt_find(T.ctable, T.cmask, Hc.done(A.hash_mask), [&](int64_t r) { return xl_same_id(T, t, L.t[0], r); });
        if (plain && stranded && contig.id >= 0 && start < T.off1[contig.id + 1] - T.off1[contig.id]) {
            const long long g1 = T.off1[contig.id] + start + 1;
            const unsigned long long m = g1 <= T.n1 ? T.map[g1] : XM_UNMAPPED;
            const long long g2 = (long long)((m >> 1) & 0xffffffffull);
            if (m != XM_UNMAPPED && g2 >= 1 && g2 <= T.off2[T.nc2]) {
                int64_t lo = 0, hi = T.nc2;                            // the last contig that starts before g2
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (T.off2[mid] < g2) lo = mid; else hi = mid;
                }
                image = true;
                const uint32_t start2 = (uint32_t)(g2 - T.off2[lo] - 1);
                const char strand2 = (m & 1ull) ? (strand == '+' ? '-' : '+') : strand;
                const char *id2 = T.ids2 + T.id_off2[lo];
                const int n_id2 = (int)(T.id_off2[lo + 1] - T.id_off2[lo]);
                KeyHash H;
                XlHash sink{&H};
                H.span(id2, n_id2); H.sep();
                rt_put_uint(sink, start2); H.sep();
                rt_put_uint(sink, start2 + 1u); H.sep();
                H.put(strand2);
                const uint64_t h = H.done(A.hash_mask);
                const KtHit hit = kt_find(A.table[1], A.mask[1], h, [&](int64_t r) {
                    if (A.hash[r] != h) return false;
                    const TabSpan R = cmp_line(A, r);
                    const char *p = A.text + A.line_start[r];
                    return R.t[0] == n_id2 && same_bytes(p, id2, n_id2) && xl_same_number(p + R.t[0] + 1, R.t[1] - R.t[0] - 1, start2) &&
                           xl_same_number(p + R.t[1] + 1, R.t[2] - R.t[1] - 1, start2 + 1u) && R.t[5] - R.t[4] == 2 && p[R.t[4] + 1] == strand2;
                });
                found = hit.id;
                looked = (int)hit.looked;
            }
        }
        if (!image) atomicAdd(&A.head->n_unaligned, 1ull);
    }
    A.match[li] = found;
    A.flag[li] = found >= 0 ? 1 : 0;
    if (looked > A.head->longest_probe) atomicMax(&A.head->longest_probe, looked);
}

// ---- the host side of the map ----
const char *xm_reason_text(int reason) {
    switch (reason) {
        case MC_CMP_DECLINE_XMFA_BYTE: return "a '\\r' or a byte >= 0x80 in the XMFA";
        case MC_CMP_DECLINE_XMFA_HEADER: return "a malformed header, or a sequence line before its block's first header";
        case MC_CMP_DECLINE_XMFA_SEQ_BYTE: return "a sequence byte that is neither '-' nor a letter";
        case MC_CMP_DECLINE_XMFA_COUNT: return "a non-gap count that disagrees with the header";
        case MC_CMP_DECLINE_XMFA_COLUMNS: return "unequal column counts in a block";
        case MC_CMP_DECLINE_XMFA_UNCLOSED: return "an entry behind the last '='";
        case MC_CMP_DECLINE_XMFA_RANGE: return "a coordinate beyond the .fai total of its genome";
        case MC_CMP_DECLINE_XMFA_GENOME: return "a genome of more than 2^31 - 2 bases, or 2^31 aligned columns or more";
        case MC_CMP_DECLINE_ROWS: return "2^31 - 2 lines or more";
        case MC_CMP_DECLINE_MEMORY: return "the alignment, its tables and the map do not fit into free device memory";
    }
    return "unknown";
}

int xm_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    return decline(c->xmfa.stats, status, "alignment reader", xm_reason_text(reason), reason, line);
}

int xm_scan(hipStream_t st, const long long *cnt, int64_t n, long long *off, long long *total) {
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, cnt, n, off, total);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the text is on the device (padded), the map allocated and all unmapped: everything behind that
int xm_run(mc_ctx *c, Pool &pool, XmArgs &A, XmHead *d_head, int32_t *status) {
    mc_xmfa_stats &S = c->xmfa.stats;
    hipStream_t st = c->stream;
    XmHead h = {};
    h.decline = CMP_NO_DECLINE;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (A.n_bytes == 0) return 0;
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, A.text, A.n_bytes, &d_head->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    A.n_nl = h.kp.n_newlines;
    if (too_many_lines(A.n_nl)) return xm_decline(c, status, MC_CMP_DECLINE_ROWS, -1);
    const size_t cap = (size_t)A.n_nl + 2;
    if (!cmp_fits(cap * (8 + 2 + 11 * 8 + 3 * 8) + ((size_t)1 << 20))) return xm_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    if (int rc = lines_starts(pool, st, A.text, A.n_bytes, A.n_nl, tile_off, &d_head->kp, &line_start)) return rc;
    A.line_start = line_start;
    if (pool.get(&A.kind, cap) || pool.get(&A.h_minus, cap) || pool.get(&A.is_hdr, cap) || pool.get(&A.is_end, cap) || pool.get(&A.cols, cap) ||
        pool.get(&A.nongap, cap) || pool.get(&A.ent_of, cap) || pool.get(&A.blk_of, cap) || pool.get(&A.col_off, cap) ||
        pool.get(&A.ng_off, cap) || pool.get(&A.h_seq, cap) || pool.get(&A.h_start, cap) || pool.get(&A.h_end, cap) ||
        pool.get(&A.hl, cap + 1) || pool.get(&A.ent_cols, cap) || pool.get(&A.blk_ent_end, cap))
        return -10;
    const unsigned line_blocks = blocks((int64_t)cap);
    hipLaunchKernelGGL(kx_lines, dim3(line_blocks), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;               // (the line count: what the scans run over)
    const int64_t L = h.kp.n_lines;
    S.n_lines = L;
    if (int rc = xm_scan(st, A.is_hdr, L, A.ent_of, &d_head->n_entries)) return rc;
    if (int rc = xm_scan(st, A.is_end, L, A.blk_of, &d_head->n_blocks)) return rc;
    if (int rc = xm_scan(st, A.cols, L, A.col_off, &d_head->n_cols_all)) return rc;
    if (int rc = xm_scan(st, A.nongap, L, A.ng_off, &d_head->n_nongap_all)) return rc;
    hipLaunchKernelGGL(kx_place, dim3(line_blocks), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kx_check, dim3(line_blocks), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_entries = h.n_entries; S.n_blocks = h.n_blocks;
    if (h.decline != CMP_NO_DECLINE) return xm_decline(c, status, decline_reason(h.decline), decline_line(h.decline));
    A.E = h.n_entries; A.B = h.n_blocks;
    if (A.E == 0) return 0;
    const size_t nb = (size_t)A.B + 1;
    if (pool.get(&A.blk_e1, nb) || pool.get(&A.blk_e2, nb) || pool.get(&A.pcols, nb) || pool.get(&A.pwords, nb) || pool.get(&A.pcol_off, nb) ||
        pool.get(&A.pword_off, nb) || pool.get(&A.blocks, nb))
        return -10;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A.blk_e1, 0x7fffffff, nb, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A.blk_e2, 0x7fffffff, nb, st));
    hipLaunchKernelGGL(kx_entries, dim3(blocks(A.E)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (A.B > 0) {
        hipLaunchKernelGGL(kx_blocks, dim3(blocks(A.B)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        if (int rc = xm_scan(st, A.pcols, A.B, A.pcol_off, &d_head->n_pcols)) return rc;
        if (int rc = xm_scan(st, A.pwords, A.B, A.pword_off, &d_head->n_words)) return rc;
    }
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.decline != CMP_NO_DECLINE) return xm_decline(c, status, decline_reason(h.decline), decline_line(h.decline));
    S.n_paired_blocks = (int64_t)h.n_paired; S.n_columns = h.n_pcols; S.n_words = h.n_words;
    if (h.n_pcols >= (1ll << 31)) return xm_decline(c, status, MC_CMP_DECLINE_XMFA_GENOME, -1);
    A.C = h.n_pcols; A.W = h.n_words;
    if (A.C == 0) return 0;
    const size_t nw = (size_t)A.W;
    if (!cmp_fits(nw * 48 + ((size_t)1 << 20))) return xm_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
    if (pool.get(&A.plane1, nw) || pool.get(&A.plane2, nw) || pool.get(&A.cnt1, nw) || pool.get(&A.cnt2, nw) || pool.get(&A.pre1, nw) ||
        pool.get(&A.pre2, nw))
        return -10;
    HIP_TRY(hipMemsetAsync(A.plane1, 0, nw * 8, st));
    HIP_TRY(hipMemsetAsync(A.plane2, 0, nw * 8, st));
    hipLaunchKernelGGL(kx_pack, dim3(line_blocks), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kx_popc, dim3(blocks(A.W)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = xm_scan(st, A.cnt1, A.W, A.pre1, &d_head->n_rank1)) return rc;
    if (int rc = xm_scan(st, A.cnt2, A.W, A.pre2, &d_head->n_rank2)) return rc;
    hipLaunchKernelGGL(kx_columns, dim3(blocks(A.C)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int xm_call(mc_ctx *c, const mc_text_source &src, int32_t seq1, int32_t seq2, int64_t n1, int64_t n2, mc_xmfa_map_view *view, int32_t *status) {
    mc_xmfa_stats &S = c->xmfa.stats;
    unsigned long long *map = nullptr;
    const int rc_call = pipeline_call(c, S, status, "alignment map", (size_t)32 << 20, [&] { if (view) *view = mc_xmfa_map_view(); }, [&](Call &K) -> int {
        hipStream_t st = c->stream;
        HIP_TRY(hipStreamSynchronize(st));
        c->xmfa.drop_map();                                            // an earlier call's map goes before this one's is made
        S.n_bytes = src.n_bytes; S.n1 = n1; S.n2 = n2;
        if (n1 > XM_COORD_CAP || n2 > XM_COORD_CAP) return xm_decline(c, status, MC_CMP_DECLINE_XMFA_GENOME, -1);
        const size_t n_map = (size_t)n1 + 1;
        if (!cmp_fits((size_t)src.n_bytes + 4096 + n_map * (view ? 17 : 8))) return xm_decline(c, status, MC_CMP_DECLINE_MEMORY, -1);
        map = c->xmfa.allocs.get<unsigned long long>(n_map);
        if (!map) return -10;
        HIP_TRY(hipMemsetAsync(map, 0xff, n_map * 8, st));
        Pool &pool = K.pool;
        char *d_text = nullptr;
        if (int rc = K.feed.put(pool, src, &d_text)) return rc;
        K.feed.times(S, K.t0);
        const auto t_kernels = std::chrono::steady_clock::now();
        XmHead *d_head = nullptr, h = {};
        XmArgs A = {};
        A.text = d_text; A.n_bytes = src.n_bytes; A.seq1 = seq1; A.seq2 = seq2; A.n1 = n1; A.n2 = n2; A.map = map;
        int rc = pool.get(&d_head, 1);
        A.head = d_head;
        if (rc == 0) rc = xm_run(c, pool, A, d_head, status);
        if (rc == 0 && *status == 0) {
            if (view && (pool.get(&A.view_g2, n_map) || pool.get(&A.view_flip, n_map))) rc = -10;
            if (rc == 0) {
                hipLaunchKernelGGL(kx_view, dim3(std::min(blocks((int64_t)n_map), 2048u)), dim3(256), 0, st, A);
                rc = mc_hip_rc(hipGetLastError(), "kx_view");
            }
            if (rc == 0) rc = fetch_head(st, d_head, h);
            S.n_mapped = (int64_t)h.n_mapped;
            S.ms_kernels = ms_since(t_kernels);
            if (rc == 0 && view) {
                const auto t_d2h = std::chrono::steady_clock::now();
                rc = c->xmfa.g2.alloc(n_map * 8);
                if (rc == 0) rc = c->xmfa.flip.alloc(n_map);
                if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(c->xmfa.g2.p, A.view_g2, n_map * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
                if (rc == 0) rc = mc_hip_rc(hipMemcpyAsync(c->xmfa.flip.p, A.view_flip, n_map, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
                if (rc == 0) rc = mc_hip_rc(hipStreamSynchronize(st), "hipStreamSynchronize");
                S.ms_d2h = ms_since(t_d2h);
                if (rc == 0) { view->n1 = n1; view->g2 = c->xmfa.g2.get<int64_t>(); view->flip = c->xmfa.flip.get<uint8_t>(); }
            }
        } else {
            S.ms_kernels = ms_since(t_kernels);                        // a declined call too: what ran until it declined
        }
        return rc;
    });
    // a call that fails or declines leaves no map behind, however far it got: a lifted comparison asks whether one is resident
    if (rc_call != 0 || *status != 0) c->xmfa.drop_map();
    else { c->xmfa.map = map; c->xmfa.n1 = n1; c->xmfa.n2 = n2; }
    return rc_call;
}
