// mc_posset.inc -- the position set of make_bed -p on the device (included by mc_bedsum.hip, inside its unnamed namespace, between
// BsArgs and the row parser): the lines of the positions file as a table of (chrom, start, end, strand) text tuples, and the
// probe the row parser makes for (chrom, pos text, decimal digits of pos + 1, strand)  (make_bed.py:13-19,:84-96).
//   kq_parse    a lane per positions line: the class of every byte; the `len(line) > 3` rule, the newline counted; strip() (blanks
//               and tabs: the only whitespace a line may still hold); the first four tab-separated fields; a 64-bit hash of them.
//               A line with fewer than four fields is no tuple a row can equal: it is left out
//   kq_insert   the tuples into a key table (kt_claim, mc_textdev.h; ids are lines): a line whose four fields equal those of the
//               slot's line byte for byte is a duplicate and stops there
//   bq_wanted   the row's probe (kt_find): the same hash (the digits of pos + 1 are generated into it, never stored), then the bytes.
//               Field 3 of a tuple equals str(int(pos) + 1) iff it is that number written without a leading zero

struct BqLine { int sb, t0, t1, t2, e3; bool ok; };      // offsets from the line start: the stripped begin, three tabs, the end of field 4

__device__ __forceinline__ BqLine bq_line(const BsArgs &A, int64_t li) {
    const uint4 r = A.p_line[li];
    BqLine L;
    L.sb = (int)(r.x & 0xffffu); L.t0 = (int)(r.x >> 16); L.t1 = (int)(r.y & 0xffffu); L.t2 = (int)(r.y >> 16);
    L.e3 = (int)(r.z & 0xffffu); L.ok = (r.z >> 16) != 0u;
    return L;
}

__global__ __launch_bounds__(256) void kq_parse(BsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.p_lines) return;
    const int64_t b = A.p_start[li];
    const int64_t e_nl = li < A.p_nl ? (int64_t)A.p_start[li + 1] : A.p_bytes;      // behind the newline, if the line has one
    const int64_t e = li < A.p_nl ? e_nl - 1 : A.p_bytes;
    A.p_line[li] = make_uint4(0u, 0u, 0u, 0u);
    A.p_hash[li] = 0;
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_BED_DECLINE_POS_LONG_LINE); return; }
    const char *t = A.ptext + b;
    const int len = (int)(e - b);
    ByteClass bad;
    for (int i = 0; i < len; ++i) bad.see((unsigned char)t[i]);
    if (bad.hi) { line_flag(&A.head->decline, li, MC_BED_DECLINE_POS_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline, li, MC_BED_DECLINE_POS_CONTROL); return; }
    if (e_nl - b <= 3) return;                                         // len(line) > 3, the newline counted
    int sb = 0, se = len;
    while (sb < se && (t[sb] == ' ' || t[sb] == '\t')) ++sb;
    while (se > sb && (t[se - 1] == ' ' || t[se - 1] == '\t')) --se;
    int t0 = 0, t1 = 0, t2 = 0, e3 = se, nt = 0;
    for (int i = sb; i < se && nt < 4; ++i)
        if (t[i] == '\t') {
            t0 = nt == 0 ? i : t0; t1 = nt == 1 ? i : t1; t2 = nt == 2 ? i : t2; e3 = nt == 3 ? i : e3;
            ++nt;
        }
    if (nt < 3) return;                                                // fewer than four fields
    KeyHash H;
    H.span(t + sb, t0 - sb); H.sep();
    H.span(t + t0 + 1, t1 - t0 - 1); H.sep();
    H.span(t + t1 + 1, t2 - t1 - 1); H.sep();
    H.span(t + t2 + 1, e3 - t2 - 1);
    A.p_hash[li] = H.done(A.hash_mask);
    A.p_line[li] = make_uint4((uint32_t)sb | ((uint32_t)t0 << 16), (uint32_t)t1 | ((uint32_t)t2 << 16), (uint32_t)e3 | (1u << 16), 0u);
}

__device__ __forceinline__ bool bq_same_tuple(const BsArgs &A, int64_t a, int64_t b) {
    const BqLine La = bq_line(A, a), Lb = bq_line(A, b);
    if (La.t0 - La.sb != Lb.t0 - Lb.sb || La.t1 - La.t0 != Lb.t1 - Lb.t0 || La.t2 - La.t1 != Lb.t2 - Lb.t1 || La.e3 - La.t2 != Lb.e3 - Lb.t2)
        return false;
    // (equal field lengths: the four fields with the tabs between them are one span of equal length)
    return same_bytes(A.ptext + A.p_start[a] + La.sb, A.ptext + A.p_start[b] + Lb.sb, La.e3 - La.sb);
}

__global__ __launch_bounds__(256) void kq_insert(BsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.p_lines || !bq_line(A, li).ok) return;
    const uint64_t h = A.p_hash[li];
    // (a tuple listed twice finds its slot taken and stops there)
    if (kt_claim(A.p_table, A.p_mask, h, li, [&](int64_t r) { return A.p_hash[r] == h && bq_same_tuple(A, li, r); }).slot < 0)
        line_flag(&A.head->decline, li, MC_BED_DECLINE_TABLE);
}

// is (chrom, pos text, str(pos + 1), strand) of the row at t listed?  t0 .. t5: the row's tabs, pos: its position as an integer
__device__ __forceinline__ bool bq_wanted(const BsArgs &A, const char *t, int t0, int t1, int t2, int t4, int t5, uint32_t pos) {
    const uint32_t end = pos + 1u;
    KeyHash H;
    H.span(t, t0); H.sep();
    H.span(t + t1 + 1, t2 - t1 - 1); H.sep();
    rt_put_uint(H, end); H.sep();
    H.span(t + t4 + 1, t5 - t4 - 1);
    const uint64_t h = H.done(A.hash_mask);
    return kt_find(A.p_table, A.p_mask, h, [&](int64_t r) {              // (the table is complete: kq_insert ran before)
        const BqLine L = bq_line(A, r);
        const char *q = A.ptext + A.p_start[r];
        if (!(A.p_hash[r] == h && L.t0 - L.sb == t0 && L.t1 - L.t0 == t2 - t1 && L.e3 - L.t2 == t5 - t4 &&
              same_bytes(q + L.sb, t, t0) && same_bytes(q + L.t0 + 1, t + t1 + 1, t2 - t1 - 1) && same_bytes(q + L.t2 + 1, t + t4 + 1, t5 - t4 - 1)))
            return false;
        const int nd = L.t2 - L.t1 - 1;                                // field 3 == str(end): 1-10 digits, no leading zero, the same number
        bool same = nd >= 1 && nd <= 10 && q[L.t1 + 1] != '0';
        uint64_t v = 0;
        for (int i = 0; i < nd && same; ++i) {
            const unsigned d = (unsigned)(unsigned char)q[L.t1 + 1 + i] - '0';
            same = d <= 9u;
            v = v * 10u + d;
        }
        return same && v == (uint64_t)end;
    }).slot >= 0;
}
