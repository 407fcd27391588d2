// mc_sitegroup.inc -- the lines of one or two .diffs files grouped by site on the GPU: what compare_currents (mc_curcompare.inc, two
// files) and cluster_sites (mc_sitecluster.inc, one file) start from, and the tail both end with.  Part of the mc_bedcompare.hip unit,
// included in front of mc_curcompare.inc.  A site is a key (chrom, pos, strand); it is kept where it has -d rows in every file.  The
// stage's argument block (SgArgs) is a member of each pipeline's own, its head (SgHead) the first member of each pipeline's head: one
// copy fetches both.  The steps (L lines, S kept sites, R their rows):
//   kp_count / kp_scan / kp_starts   line starts (mc_lines.h)
//   kn_parse     a lane per line, 256 lines of a workgroup staged in LDS (staged_lines): ByteClass, the 6 or 7 tabs, the KeyHash of chrom,
//                pos and strand, the comma count, every number's grammar (mc_decimal.h: the host calls float() on all of them), the
//                plain-digit test of pos; the lines that start before the second file's text (n_lines1)
//   kn_group     ONE key table for all lines (kt_claim, byte comparison).  The line that claimed the slot names the key; per key the smallest
//                line of the first file (atomicMin) and the rows of each file (atomicAdd), integers all: nothing depends on arrival
//   kn_select<files> / kp_scan   a key is kept where it has -d rows in every file; its smallest line of the first file is its head.
//                The scan over the head flags numbers the kept sites in the order of their first rows (no atomic decides an order)
//   kn_sites<files> / kp_scan per file   per site: head line, rows per file; the files' row offsets
//   kn_claim / kn_place   rows into their (site, file) bucket in arrival order (atomicAdd), then every row's RANK among its bucket's
//                line numbers -> the bucket in ascending line order whatever the arrival.  A lane per row reads its bucket once: n1^2 +
//                n2^2 reads a site, the one work not linear in the file -- 2^25 at the comparison's cap, beside kc_rank_large's 2^26 compares
// One file is `files == 1`, not a comparison with an empty control: off2 is the text's end, so kn_parse counts every line into n_lines1
// and no line is the second file's; key_cnt has one count a key, and cnt2, off2r and n_ry do not exist (cu_row reads them for a line at
// or behind n_lines1 alone).  The host sequence is three phases -- SgRun::keys, sites, place -- with the pipeline's own allocations,
// kernels and its fetch of the head between them: sites and place end without a host synchronisation.  sg_outputs is the tail.
// Resources (tools/kres.py, gfx950; none spills or uses scratch, none uses static LDS, every one runs at 8 waves a SIMD):
//   kn_parse    44 VGPRs, 48 KB + 16 bytes of dynamic LDS (the staged lines: three workgroups a CU of its 160 KB)
//   kn_group    41    kn_claim  10    kn_place  12    kn_select<2>  10    kn_select<1>  8    kn_sites<2>  14    kn_sites<1>  12
#include <functional>

constexpr int CU_STAGE = 48 * 1024;          // LDS a workgroup of kn_parse stages its 256 lines in (as kb_parse)
constexpr unsigned CU_NONE = 0xffffffffu;

struct SgHead {                              // what grouping reports (device side; copied to the host as it is)
    KpHead kp;
    unsigned long long decline;              // min over the offending lines of line << 8 | reason (~0: none); the pipeline's kernels flag here too
    long long n_lines1;                      // lines that start before the second file's text (one file: all)
    long long n_sites, n_rx, n_ry;           // totals of the scans
    unsigned long long n_keys;
    int longest_probe, deepest;
};

struct SgArgs {
    const char *text;
    int64_t n_bytes, off2, n_nl, n_lines, n_lines1;      // off2: where the second file's text begins (one file: n_bytes)
    const long long *line_start;
    SgHead *head;
    int files, depth, c;                     // files: 1 or 2; c: values a line has beside the read quality
    long long pooled_cap;                    // rows a kept site may have in its files together (0: as many as there are)
    // per line
    uint4 *span;                             // tabs_pack (t6 = len in a 7-field row); 0: not a line the table takes
    uint64_t *hash;
    uint32_t *n_vals, *rep;                  // rep: the line that names the line's key
    long long *flag, *site_of;               // first file's lines: 1 at a kept site's head, the scan
    uint64_t hash_mask, mask;
    unsigned long long *table;
    // per key, at the line that names it
    uint32_t *key_first, *key_cnt;           // smallest line of the first file; rows of the first file [rep], of the second [cap + rep]
    int32_t *key_site;                       // the kept site's number, -1: none
    int64_t cap;
    // per site
    int64_t S;
    long long *head_line, *cnt1, *cnt2, *off1, *off2r;
    unsigned int *fill;                      // [2 S]
    // per row of a kept site: the first file's rows [0, n_rx), the second's [n_rx, n_rx + n_ry)
    int64_t n_rx, n_ry;
    uint32_t *claimed, *rows;                // line numbers in arrival order, in ascending order
};

// per site: the lengths and places of its row and its bed line; the two outputs (each pipeline's block has one beside its SgArgs)
struct SgOut { long long *row_len, *row_off, *bed_len, *bed_off; char *out, *bed; };

__device__ __forceinline__ TabSpan cu_line(const SgArgs &A, int64_t li) { return tabs_unpack(A.span[li]); }

// One line: t[x - adj] is byte x of the text (the staged piece in LDS, or the text itself with adj = 0)
__device__ __forceinline__ void cu_parse_line(const SgArgs &A, const char *t, const int64_t adj, const int64_t li) {
    const int64_t b = A.line_start[li] - adj;
    const int64_t e = (li < A.n_nl ? A.line_start[li + 1] - 1 : A.n_bytes) - adj;
    A.span[li] = make_uint4(0u, 0u, 0u, 0u);
    A.hash[li] = 0;
    A.n_vals[li] = 0;
    A.rep[li] = CU_NONE;
    if (b + adj < A.off2 && (li + 1 >= A.n_lines || (int64_t)A.line_start[li + 1] >= A.off2)) A.head->n_lines1 = li + 1;      // the first text's last line alone
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_LONG_LINE); return; }
    const int len = (int)(e - b);
    int tab[7] = {0, 0, 0, 0, 0, 0, 0}, nt = 0, commas = 0;
    ByteClass bad;
    KeyHash H;
    for (int i = 0; i < len; ++i) {
        const unsigned ch = (unsigned char)t[b + i];
        bad.see(ch);
        if (ch == '\t') {
#pragma unroll
            for (int k = 0; k < 7; ++k) tab[k] = nt == k ? i : tab[k];
            if (nt == 0 || nt == 2) H.sep();                          // behind chrom, behind pos
            ++nt;
        } else if (nt == 0 || nt == 2 || nt == 5) {                   // chrom, pos, strand
            H.put((char)ch);
        } else if (nt == 4) {
            commas += ch == ',';
        }
    }
    if (bad.hi) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CONTROL); return; }
    if (nt != 6 && nt != 7) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CUR_FIELDS); return; }
    if (nt == 6) tab[6] = len;
    // every number of the line, the read quality too: the host calls float() on all of them
    bool bad_number = false;
    for (int p = tab[3] + 1, tb = tab[3] + 1; p <= tab[4]; ++p)
        if (p == tab[4] || t[b + p] == ',') {
            double d;
            bad_number |= !dc_parse(t + b + tb, p - tb, &d);
            tb = p + 1;
        }
    if (bad_number) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_NUMBER); return; }
    if (commas + 1 != A.c + 1 || A.c < 1) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CUR_VALUES); return; }
    const int pn = tab[2] - tab[1] - 1;
    bool plain = pn >= 1 && pn <= 9 && !(pn > 1 && t[b + tab[1] + 1] == '0');
    for (int i = tab[1] + 1; i < tab[2]; ++i) plain = plain && (unsigned)((unsigned char)t[b + i]) - '0' <= 9u;
    if (!plain) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_CUR_POS); return; }
    A.hash[li] = H.done(A.hash_mask);
    A.n_vals[li] = (uint32_t)commas + 1u;
    A.span[li] = tabs_pack(tab, len);
}

__global__ __launch_bounds__(256) void kn_parse(SgArgs A) {
    (void)staged_lines<CU_STAGE>(A.text, A.n_bytes, A.line_start, A.n_lines, A.n_nl,
                                 [&](const char *t, int64_t adj, int64_t li) { cu_parse_line(A, t, adj, li); });
}

// (chrom, pos, strand) of lines a and b, byte for byte
__device__ __forceinline__ bool cu_same_key(const SgArgs &A, int64_t a, int64_t b) {
    const TabSpan La = cu_line(A, a), Lb = cu_line(A, b);
    if (La.t[0] != Lb.t[0] || La.t[2] - La.t[1] != Lb.t[2] - Lb.t[1] || La.t[5] - La.t[4] != Lb.t[5] - Lb.t[4]) return false;
    const char *pa = A.text + A.line_start[a], *pb = A.text + A.line_start[b];
    return same_bytes(pa, pb, La.t[0]) && same_bytes(pa + La.t[1] + 1, pb + Lb.t[1] + 1, La.t[2] - La.t[1] - 1) &&
           same_bytes(pa + La.t[4] + 1, pb + Lb.t[4] + 1, La.t[5] - La.t[4] - 1);
}

__global__ __launch_bounds__(256) void kn_group(SgArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines || cu_line(A, li).len == 0) return;            // (a line kn_parse left out: it has declined the file)
    const uint64_t h = A.hash[li];
    const KtHit hit = kt_claim(A.table, A.mask, h, li, [&](int64_t r) { return A.hash[r] == h && cu_same_key(A, li, r); });
    if (hit.slot < 0 || hit.id < 0 || hit.id >= A.n_lines) { line_flag(&A.head->decline, li, MC_CMP_DECLINE_TABLE); return; }
    const int64_t rep = hit.id;
    A.rep[li] = (uint32_t)rep;
    const bool native = li < A.n_lines1;
    atomicAdd(&A.key_cnt[(native ? 0 : A.cap) + rep], 1u);
    if (native) atomicMin(&A.key_first[rep], (uint32_t)li);
    if (hit.claimed) atomicAdd(&A.head->n_keys, 1ull);
    const int looked = (int)(hit.looked > 0x7fffffffull ? 0x7fffffffull : hit.looked);
    if (looked > A.head->longest_probe) atomicMax(&A.head->longest_probe, looked);
}

// a line of the first file is the head of a kept site: the smallest such line of a key with -d rows in every file
template <int FILES>
__global__ __launch_bounds__(256) void kn_select(SgArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1) return;
    long long keep = 0;
    const uint32_t rep = A.rep[li];
    if (rep != CU_NONE && A.key_first[rep] == (uint32_t)li) {
        const long long c1 = A.key_cnt[rep], c2 = FILES == 2 ? A.key_cnt[A.cap + rep] : 0;
        if (c1 >= A.depth && (FILES == 1 || c2 >= A.depth)) {
            keep = 1;
            if (A.pooled_cap > 0 && c1 + c2 > A.pooled_cap) line_flag(&A.head->decline, li, MC_CMP_DECLINE_DEPTH);
            const int deep = (int)(c1 + c2 > 0x7fffffffll ? 0x7fffffffll : c1 + c2);
            if (deep > A.head->deepest) atomicMax(&A.head->deepest, deep);
        }
    }
    A.flag[li] = keep;
}

template <int FILES>
__global__ __launch_bounds__(256) void kn_sites(SgArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines1 || A.flag[li] == 0) return;
    const long long s = A.site_of[li];
    if (s < 0 || s >= A.S) return;                                     // (cannot be: the scan counted these lines)
    const uint32_t rep = A.rep[li];
    A.head_line[s] = li;
    A.cnt1[s] = A.key_cnt[rep];
    if (FILES == 2) A.cnt2[s] = A.key_cnt[A.cap + rep];
    A.key_site[rep] = (int32_t)s;
}

// the site of line li (-1: its key is not kept), which file it is of, where its bucket starts and how many rows it has
struct CuRow { long long s, off, n; bool control; };
__device__ __forceinline__ CuRow cu_row(const SgArgs &A, int64_t li) {
    CuRow r{-1, 0, 0, li >= A.n_lines1};
    const uint32_t rep = A.rep[li];
    if (rep == CU_NONE) return r;
    const long long s = A.key_site[rep];
    if (s < 0 || s >= A.S) return r;
    r.s = s;
    r.off = r.control ? A.n_rx + A.off2r[s] : A.off1[s];
    r.n = r.control ? A.cnt2[s] : A.cnt1[s];
    return r;
}

__global__ __launch_bounds__(256) void kn_claim(SgArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines) return;
    const CuRow r = cu_row(A, li);
    if (r.s < 0) return;
    const long long k = atomicAdd(&A.fill[2 * r.s + (r.control ? 1 : 0)], 1u);
    if (k < r.n && r.off + k < A.n_rx + A.n_ry) A.claimed[r.off + k] = (uint32_t)li;      // (always: the counts are kn_group's)
}

// the rank of a row's line number among its bucket's: its place in ascending line order
__global__ __launch_bounds__(256) void kn_place(SgArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines) return;
    const CuRow r = cu_row(A, li);
    if (r.s < 0 || r.off + r.n > A.n_rx + A.n_ry) return;
    long long rank = 0;
    for (long long k = 0; k < r.n; ++k) rank += A.claimed[r.off + k] < (uint32_t)li;
    A.rows[r.off + rank] = (uint32_t)li;
}

// value j of line li's list (the comma walk, mc_decimal.h); a value the reader declines flags the line and reads as 0
__device__ __forceinline__ double cu_value(const SgArgs &A, int64_t li, int j) {
    const TabSpan L = cu_line(A, li);
    const char *t = A.text + A.line_start[li];
    int tb = L.t[3] + 1, k = 0, p = L.t[3] + 1;
    for (; p < L.t[4]; ++p)
        if (t[p] == ',') {
            if (k == j) break;
            ++k; tb = p + 1;
        }
    double d = 0.0;
    if (k != j || !dc_parse(t + tb, p - tb, &d)) line_flag(&A.head->decline, li, MC_CMP_DECLINE_NUMBER);
    return d;
}

__device__ __forceinline__ uint32_t cu_pos(const char *p, const TabSpan &L) {
    uint32_t pos = 0;
    for (int i = L.t[1] + 1; i < L.t[2]; ++i) pos = pos * 10u + (uint32_t)(p[i] - '0');
    return pos;
}

// what every row and bed line begins with, from the site's head line p: chrom pos pos+1 context, a tab behind each
template <class Sink>
__device__ __forceinline__ void cu_put_prefix(const char *p, const TabSpan &L, Sink &o) {
    for (int i = 0; i <= L.t[0]; ++i) o.put(p[i]);                     // chrom and its tab
    for (int i = L.t[1] + 1; i <= L.t[2]; ++i) o.put(p[i]);            // pos
    rt_put_uint(o, cu_pos(p, L) + 1u); o.put('\t');
    for (int i = L.t[2] + 1; i <= L.t[3]; ++i) o.put(p[i]);            // context
}

// strand and its tab, the rows n, `end`
template <class Sink>
__device__ __forceinline__ void cu_put_strand_n(const char *p, const TabSpan &L, long long n, char end, Sink &o) {
    for (int i = L.t[4] + 1; i <= L.t[5]; ++i) o.put(p[i]);
    rt_put_uint(o, (uint32_t)n); o.put(end);
}

// the bed line of site s: chrom pos pos+1 context value strand n (the first file's rows)
template <class Sink>
__device__ __forceinline__ void cu_put_bed(const SgArgs &A, int64_t s, double value, Sink &o) {
    const long long li = A.head_line[s];
    const TabSpan L = cu_line(A, li);
    const char *p = A.text + A.line_start[li];
    cu_put_prefix(p, L, o);
    rt_put_num(o, rt_num_of(value)); o.put('\t');
    cu_put_strand_n(p, L, A.cnt1[s], '\n', o);
}

// A lane per site writes its row and its bed line where the scans put them.  Args: a pipeline's block with g (SgArgs), o (SgOut), its
// head (out_bytes, bed_bytes) and put_row / bed_value of its own
template <class Args>
__device__ __forceinline__ void sg_write_site(const Args &A) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.g.S) return;
    const long long at = A.o.row_off[s], len = A.o.row_len[s];
    if (len > 0 && at >= 0 && at + len <= A.head->out_bytes) {         // (always: the scan counted these bytes)
        RtStore store{A.o.out + at};
        put_row(A, s, store);
    }
    const long long bat = A.o.bed_off[s], blen = A.o.bed_len[s];
    if (blen > 0 && bat >= 0 && bat + blen <= A.head->bed_bytes) {
        RtStore store{A.o.bed + bat};
        cu_put_bed(A.g, s, bed_value(A, s), store);
    }
}

// One grouping on the host.  The pipeline fills A.text, n_bytes, files, off2 (two files), depth, c and pooled_cap and says how it declines:
// decline(reason, line of the text or -1).  A phase returns 0: go on, 1: the call is over (a decline has set the status, or the text has
// no site), < 0: an error.  What the stats say of grouping is in h where the head has it; n_lines, n_lines2 and n_slots stand here
struct SgRun {
    Pool &pool; hipStream_t st; SgArgs &A;
    SgHead &h;                               // the host's copy: the g of the pipeline's own
    std::function<int(int, long long)> decline;
    int64_t n_lines = 0, n_lines2 = 0, n_slots = 0;

    int stop(int reason, long long line = -1) { decline(reason, line); return 1; }
    int stop_head() { return stop(decline_reason(h.decline), decline_line(h.decline)); }
    // Phase 1: the head block (d_head: the g of the pipeline's own block of head_bytes, zero but for the decline word), line starts,
    // parse, the key table, the kept sites numbered: A.S
    int keys(SgHead *d_head, size_t head_bytes) {
        A.head = d_head;
        if (A.files == 1) A.off2 = A.n_bytes;
        h = SgHead(); h.decline = CMP_NO_DECLINE;
        HIP_TRY(hipMemsetAsync(d_head, 0, head_bytes, st));
        HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
        long long *tile_off = nullptr, *line_start = nullptr;
        if (int rc = lines_count(pool, st, A.text, A.n_bytes, &d_head->kp, &tile_off)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        const int64_t n_nl = h.kp.n_newlines;
        if (too_many_lines(n_nl)) return stop(MC_CMP_DECLINE_ROWS);
        const size_t cap = (size_t)n_nl + 2;
        // per line: its start, span, hash, n_vals, rep, flag, site_of, key_first, a count a file, key_site
        if (!cmp_fits(cap * (8 + 16 + 8 + 4 + 4 + 8 + 8 + 4 + 4 * (size_t)A.files + 4) + ((size_t)1 << 20))) return stop(MC_CMP_DECLINE_MEMORY);
        if (int rc = lines_starts(pool, st, A.text, A.n_bytes, n_nl, tile_off, &d_head->kp, &line_start)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        const int64_t L = h.kp.n_lines;
        if (L <= 0 || L > (int64_t)cap) return 1;
        n_lines = L;
        A.n_nl = n_nl; A.n_lines = L; A.line_start = line_start; A.cap = (int64_t)cap;
        A.hash_mask = cmp_hash_mask();
        if (pool.get(&A.span, cap) || pool.get(&A.hash, cap) || pool.get(&A.n_vals, cap) || pool.get(&A.rep, cap) || pool.get(&A.flag, cap) ||
            pool.get(&A.site_of, cap) || pool.get(&A.key_first, cap) || pool.get(&A.key_cnt, (size_t)A.files * cap) || pool.get(&A.key_site, cap))
            return -10;
        hipLaunchKernelGGL(kn_parse, dim3(blocks(L)), dim3(256), CU_STAGE + 16, st, A);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;
        const int64_t L1 = h.n_lines1;
        n_lines2 = L - L1;
        if (h.decline != CMP_NO_DECLINE) return stop_head();
        A.n_lines1 = L1;
        if (L1 == 0 || (A.files == 2 && L1 == L)) return 1;
        A.mask = table_slots(L, 64, "MCALLER_CMP_TABLE_SLOTS") - 1;
        n_slots = (int64_t)A.mask + 1;
        if (!cmp_fits((A.mask + 1) * 8 + ((size_t)1 << 20))) return stop(MC_CMP_DECLINE_MEMORY);
        if (int rc = table_get(pool, st, &A.table, A.mask + 1)) return rc;
        HIP_TRY(hipMemsetAsync(A.key_first, 0xff, cap * 4, st));
        HIP_TRY(hipMemsetAsync(A.key_cnt, 0, (size_t)A.files * cap * 4, st));
        HIP_TRY(hipMemsetAsync(A.key_site, 0xff, cap * 4, st));
        hipLaunchKernelGGL(kn_group, dim3(blocks(L)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(A.files == 2 ? kn_select<2> : kn_select<1>, dim3(blocks(L1)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.flag, L1, A.site_of, &d_head->n_sites);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.decline != CMP_NO_DECLINE) return stop_head();
        if (h.n_sites <= 0) return 1;
        A.S = h.n_sites;
        return 0;
    }

    // Phase 2: the per-site columns and the files' row offsets (the scans' totals go to the head's n_rx, n_ry: the pipeline fetches them
    // with its own).  extra: the bytes of the pipeline's own columns, counted with the stage's.  No host synchronisation
    int sites(size_t extra) {
        const size_t ns = (size_t)A.S;
        const bool two = A.files == 2;
        if (!cmp_fits(ns * ((two ? 5 : 3) * 8 + 2 * 4) + extra + ((size_t)1 << 20))) return stop(MC_CMP_DECLINE_MEMORY);
        if (pool.get(&A.head_line, ns) || pool.get(&A.cnt1, ns) || pool.get(&A.off1, ns) || pool.get(&A.fill, 2 * ns) ||
            (two && (pool.get(&A.cnt2, ns) || pool.get(&A.off2r, ns))))
            return -10;
        HIP_TRY(hipMemsetAsync(A.fill, 0, 2 * ns * 4, st));
        hipLaunchKernelGGL(two ? kn_sites<2> : kn_sites<1>, dim3(blocks(A.n_lines1)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt1, A.S, A.off1, &A.head->n_rx);
        if (two) hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt2, A.S, A.off2r, &A.head->n_ry);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // Phase 3, behind the pipeline's fetch of the head: the kept sites' rows into their buckets, in ascending line order.  extra as in
    // sites.  No host synchronisation
    int place(size_t extra) {
        A.n_rx = h.n_rx; A.n_ry = h.n_ry;
        const size_t nr = (size_t)(A.n_rx + A.n_ry);
        if (!cmp_fits(nr * 8 + extra + ((size_t)1 << 20))) return stop(MC_CMP_DECLINE_MEMORY);
        if (pool.get(&A.claimed, nr + 1) || pool.get(&A.rows, nr + 1)) return -10;
        HIP_TRY(hipMemsetAsync(A.claimed, 0xff, (nr + 1) * 4, st));
        HIP_TRY(hipMemsetAsync(A.rows, 0xff, (nr + 1) * 4, st));
        hipLaunchKernelGGL(kn_claim, dim3(blocks(A.n_lines)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kn_place, dim3(blocks(A.n_lines)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        return 0;
    }
};

// The tail of a pipeline: its size kernel, the two scans, the head (h: the whole of it, fetched here), the two outputs written by its
// write kernel and copied into the context's pinned blocks; the outputs' stats and the result's pointers.  Returns as a phase does
template <class Args, class Head, class Stats, class Res>
int sg_outputs(mc_ctx *c, SgRun &R, Args &A, Head *d_head, Head &h, void (*k_size)(Args), void (*k_write)(Args), Grown &out, Grown &bed,
               Stats &S, Res *res) {
    static_assert(offsetof(Head, g) == 0, "SgRun::keys clears the head from its g on, and fetches that");
    hipStream_t st = R.st;
    const int64_t NS = A.g.S;
    hipLaunchKernelGGL(k_size, dim3(blocks(NS)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.o.row_len, NS, A.o.row_off, &d_head->out_bytes);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.o.bed_len, NS, A.o.bed_off, &d_head->bed_bytes);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.g.decline != CMP_NO_DECLINE) return R.stop_head();
    const size_t ob = (size_t)h.out_bytes, bb = (size_t)h.bed_bytes;
    if (!cmp_fits(ob + bb + ((size_t)1 << 20))) return R.stop(MC_CMP_DECLINE_MEMORY);
    if (R.pool.get(&A.o.out, ob + 1) || R.pool.get(&A.o.bed, bb + 1)) return -10;
    hipLaunchKernelGGL(k_write, dim3(blocks(NS)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = fetch_out(c, out, A.o.out, ob, &res->out, &res->n_out)) return rc;
    if (int rc = fetch_out(c, bed, A.o.bed, bb, &res->bed, &res->n_bed)) return rc;
    S.ms_d2h = ms_since(t_d2h);
    S.n_out_bytes = (int64_t)ob; S.n_bed_bytes = (int64_t)bb;
    return 0;
}
