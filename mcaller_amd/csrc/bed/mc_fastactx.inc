// mc_fastactx.inc -- the contexts of make_bed --ref on the device (included by mc_bedsum.hip, inside its unnamed namespace, behind
// the grouping kernels): make_bed.py:36-48 over refmark.read_fasta -- a record starts at a '>' in column 0, text before the first one
// is ignored, the id is the first whitespace-separated token of the title line, the sequence is every byte behind the title line
// that is no whitespace, and of several records with one id the LAST counts (dict()).  An entry's context is seq[p - 20 : p + 21]
// with Python's slice rule, upper-cased, and on '-' complemented over ACGTNM and reversed; it replaces the row's context in the GFF
// attributes only.  The FASTA text goes up like the positions text; kp_count / kp_scan / kp_starts give its line starts.
//   kf_lines     a wave per line: the class of every byte (a byte >= 0x80, a control byte: declined), whether it is a title, its
//                number of bytes and whether all are letters; a title's id span and 64-bit hash
//   kp_scan x 2  over the lines: sequence bytes before a line (its place in the packed array), titles before it (its record)
//   kf_pack      a wave per line: a title notes where its record begins; a sequence line of a record goes upper-cased into the
//                packed array -- with a byte that is no letter (a blank, a digit, '*', '-') it declines the file: the host strips
//                whitespace there and keeps the rest, the device leaves both to the host
//   kf_ids       a lane per record: its id into a key table (kt_claim, mc_textdev.h; ids of the table are records); atomicMax of the
//                record number on the slot, so the last record of an id wins whatever the order of arrival
//   kf_context   a lane per entry (its first row): the table probed with the chrom bytes, the slice rule -> where the window begins
//                in the packed array, its length (0 .. 41) and whether it is reversed; bs_put_context writes it from there
//                (complemented and reversed on the fly) for the sizing pass and kb_write.  On '-' a letter outside ACGTNM declines
//                (the host's KeyError, written entry or not); so does a WRITTEN entry whose contig the FASTA lacks

__device__ __forceinline__ bool bf_blank(unsigned c) { return c == ' ' || c == '\t'; }      // the whitespace a text that is not declined holds in a line

__global__ __launch_bounds__(256) void kf_lines(BsArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t li = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (li >= A.f_lines) return;
    const int64_t b = A.f_start[li];
    const int64_t e = li < A.f_nl ? (int64_t)A.f_start[li + 1] - 1 : A.f_bytes;
    const char *t = A.ftext;
    const bool title = e > b && t[b] == '>';
    ByteClass bad;
    bool other = false;
    for (int64_t i = b + lane; i < e; i += 64) {
        const unsigned c = (unsigned char)t[i];
        bad.see(c);
        other |= !((c | 0x20u) >= 'a' && (c | 0x20u) <= 'z');
    }
    const bool any_hi = __ballot(bad.hi) != 0ull, any_ctrl = __ballot(bad.ctrl) != 0ull, any_other = __ballot(other) != 0ull;
    if (lane != 0) return;
    if (any_hi) line_flag(&A.head->decline, li, MC_BED_DECLINE_REF_HIGH_BYTE);
    else if (any_ctrl) line_flag(&A.head->decline, li, MC_BED_DECLINE_REF_CONTROL);
    A.f_cnt[li] = title ? 0 : e - b;
    A.f_cnt[A.f_lines + li] = title ? 1 : 0;
    A.f_bad[li] = (uint8_t)(!title && any_other);
    uint32_t ib = 0, in = 0;
    KeyHash H;
    if (title && !any_hi && !any_ctrl) {
        int64_t i = b + 1;
        while (i < e && bf_blank((unsigned char)t[i])) ++i;
        const int64_t i0 = i;
        while (i < e && !bf_blank((unsigned char)t[i])) ++i;
        ib = (uint32_t)(i0 - b); in = (uint32_t)(i - i0);
        H.span(t + i0, (int)in);
    }
    A.f_idb[li] = ib; A.f_idn[li] = in;
    A.f_hash[li] = H.done(A.hash_mask);
}

__global__ __launch_bounds__(256) void kf_pack(BsArgs A, long long n_rec, long long total) {
    const int lane = threadIdx.x & 63;
    const int64_t li = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (li >= A.f_lines) return;
    const long long rec = A.f_off[A.f_lines + li];                     // titles before this line
    const long long at = A.f_off[li];
    if (li == 0 && lane == 0) A.rec_begin[n_rec] = total;
    if (A.f_cnt[A.f_lines + li]) {
        if (lane == 0) { A.rec_begin[rec] = at; A.rec_line[rec] = (uint32_t)li; }
        return;
    }
    if (rec == 0) return;                                              // before the first record
    if (A.f_bad[li]) { if (lane == 0) line_flag(&A.head->decline, li, MC_BED_DECLINE_REF_SEQ_BYTE); return; }
    const int64_t b = A.f_start[li], n = A.f_cnt[li];
    for (int64_t i = lane; i < n; i += 64) A.f_seq[at + i] = (char)((unsigned char)A.ftext[b + i] & 0xdfu);      // upper case
}

__device__ __forceinline__ bool bf_same_id(const BsArgs &A, uint32_t line, const char *s, uint32_t n) {
    return A.f_idn[line] == n && same_bytes(A.ftext + A.f_start[line] + A.f_idb[line], s, (int)n);
}

__global__ __launch_bounds__(256) void kf_ids(BsArgs A, long long n_rec) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const uint32_t line = A.rec_line[r];
    const uint64_t h = A.f_hash[line];
    const char *id = A.ftext + A.f_start[line] + A.f_idb[line];
    const KtHit hit = kt_claim(A.f_table, A.f_mask, h, r, [&](int64_t q) {      // (ids of the table are records)
        const uint32_t other = A.rec_line[q];
        return A.f_hash[other] == h && bf_same_id(A, other, id, A.f_idn[line]);
    });
    if (hit.slot < 0) { line_flag(&A.head->decline, line, MC_BED_DECLINE_TABLE); return; }
    atomicMax(&A.f_win[hit.slot], (uint32_t)(r + 1));                  // claimed, or the same id again: the last record wins
}

// the record (the last of its id) whose id is s[0, n), or -1
__device__ __forceinline__ long long bf_find(const BsArgs &A, const char *s, int n) {
    KeyHash H;
    H.span(s, n);
    const uint64_t h = H.done(A.hash_mask);
    const KtHit hit = kt_find(A.f_table, A.f_mask, h, [&](int64_t q) {   // (the table is complete: kf_ids ran before)
        const uint32_t line = A.rec_line[q];
        return A.f_hash[line] == h && bf_same_id(A, line, s, (uint32_t)n);
    });
    return hit.slot < 0 ? -1 : (long long)A.f_win[hit.slot] - 1;
}

__global__ __launch_bounds__(256) void kf_context(BsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines || !(A.fl[li] & BS_F_COUNTED)) return;
    const uint32_t rep = A.row_ent[li];
    if (A.ent_min[rep] != (uint32_t)li) return;                        // the entry's first row speaks for it
    const TabSpan R = bs_row(A, li);
    const char *t = A.text + A.line_start[li];
    const long long r = A.n_rec > 0 ? bf_find(A, t, R.t[0]) : -1;
    if (r < 0) {
        if (bs_selected(A, rep)) line_flag(&A.head->decline, li, MC_BED_DECLINE_REF_CONTIG);
        return;
    }
    const long long begin = A.rec_begin[r], L = A.rec_begin[r + 1] - begin;
    long long start = (long long)A.pos[li] - 20, stop = (long long)A.pos[li] + 21;      // seq[p - 20 : p + 21]
    if (start < 0) { start += L; if (start < 0) start = 0; }
    if (start > L) start = L;
    if (stop > L) stop = L;
    const int n = stop > start ? (int)(stop - start) : 0;
    const bool rev = R.t[5] - R.t[4] - 1 == 1 && t[R.t[4] + 1] == '-';
    if (rev)
        for (int i = 0; i < n; ++i) {
            const char c = A.f_seq[begin + start + i];
            if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N' || c == 'M')) { line_flag(&A.head->decline, li, MC_BED_DECLINE_REF_LETTER); return; }
        }
    A.ctx_at[rep] = begin + start;
    A.ctx_len[rep] = (uint8_t)(n | (rev ? 0x80 : 0));
}

// the context of entry `rep` from the packed sequences (kf_context found it)
template <class Sink>
__device__ __forceinline__ void bs_put_context(const BsArgs &A, Sink &o, uint32_t rep) {
    const int n = A.ctx_len[rep] & 0x7f;
    const char *s = A.f_seq + A.ctx_at[rep];
    if (!(A.ctx_len[rep] & 0x80)) { bs_put_span(o, s, n); return; }
    for (int i = n - 1; i >= 0; --i) {
        const char c = s[i];
        o.put(c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c);      // (N and M are their own complements)
    }
}
