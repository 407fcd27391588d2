// mc_evalcalls.hip -- the evaluation file of mcaller_amd/evaluate.py, made on the GPU: the text of a `.diffs.<k>` file and of a
// labelled positions file -> the bytes of evaluate.evaluate_calls, or a decline (C ABI: mc_eval_calls, mc_eval_last_stats,
// mc_eval_release; Python: Device.eval_calls, evaluate.evaluate_calls_device, `python -m mcaller_amd.evaluate --device`).  The unit
// stands in csrc/eval/ beside csrc/bed/, csrc/compare/ and the other file pipelines: no pass runs its kernels.  Also here: the probe
// of mc_hypergeom.h's hg_masses on the device (mc_hypergeom_masses_device, a lane per case).
//
// The steps (both texts stay resident; line starts by mc_lines.h's kp_count / kp_scan / kp_starts through mc_textfeed.h):
//   ke_truth_parse   a lane per positions line, pos2label's rules: tokens are runs of bytes that are no blank or tab; fewer than 2
//                    tokens: skipped; fewer than 4: declined (the host's IndexError); tok[1] 1-18 decimal digits (int('007') == 7:
//                    the VALUE is the key); the hash of (tok[0] bytes, value, tok[2] bytes); tok[3][0] == 'm'
//   ke_truth_insert  the keys into a key table (kt_claim, mc_textdev.h; ids are lines); the LAST line of a key wins: an integer
//                    atomicMax of line + 1 on the slot's side record
//   ke_rows          a lane per .diffs line, 256 lines staged in LDS (staged_lines), judged in the host's order: 8 tab fields; the
//                    centre of the context ('M' or n_not_m; empty: declined); the position; kt_find (none: n_unlabelled, the
//                    probability is never looked at); the probability (blanks stripped, mc_decimal.h, inside [0, 1]).  A kept row:
//                    an integer atomicAdd on its slot's N, on K when label[0] == 'm'; c = #{j : p >= j / 100} (ev_bucket) into an
//                    LDS histogram [2][102], flushed with integer atomics
//   ke_sites         a lane per slot with N > 0: the site counters, the list of such slots, K / N (one fp64 division) -> c -> the
//                    "site all" histogram when N >= min_depth
//   ke_expect        the hot path: a lane per (listed site, depth) with N >= d runs hg_masses_to (two walks of the weights, no array);
//                    blockIdx.y is the depth.  Every bucket mass goes as floor(mass * 2^62) into two 64-bit integer LDS counters of
//                    its cell [class][c] -- the high 32 bits and the low 32 bits, each summed on its own: below 2^31 sites neither
//                    overflows --, the site's bound as ceil(err * 2^62) + the buckets it put (a unit each for the floor) into one
//                    per class; the LDS cells are flushed with integer atomics.  No floating-point atomic anywhere: the sums are
//                    exact integers and do not depend on the order of arrival
//   ke_finish        a lane per printed value (203 a table: 101 tpr, 101 fpr, the AUC).  Integer tables: suffix sums of the
//                    histograms; a rate and the AUC sum_j (FP_j - FP_j+1)(TP_j + TP_j+1) / (2 P N_neg) as the correctly rounded
//                    quotient of two integers below 2^63 (ev_quot: mc_decimal.h's 128-bit division and rounding) -- the host's bits.
//                    Expected tables: below
//   ke_write / kp_scan / ke_pack   a lane per line of the file: its bytes (mc_rowtext.h) at a fixed stride, the lengths scanned,
//                    the lines packed
//
// The expected tables and their bounds.  E_j = sum over the sites and over c > j of the quantised masses, an integer in units of
// 2^-62; B = the class's summed site bounds in the same unit.  For a site sum_c |q_c 2^-62 - mass[c]| <= err + (buckets put) 2^-62
// (hg_masses' bound, which counts the buckets nothing was put in, and the floor), so |E_j 2^-62 - exact E_j| <= B 2^-62 for every j.
//   B == 0 (every mass of the class trivial: each is 2^62 exactly): E_j >> 62 is a count and the rate is ev_quot(count, P), the
//       host's bits; an AUC with both classes at B == 0 is the integer table's AUC of the counts.  No tie question.
//   rate  v = fl(fl(E_j) 2^-62 / P): two roundings, |v - E_j 2^-62 / P| <= 3 u v'; the host prints fl(exact), within u of exact.
//       bound = 1.0000001 (B 2^-62 / P) + 8 u v  (the factor covers fl(B) and the bound's own operations).
//   AUC   every term m_j (TP_j + TP_j+1) is non-negative (m_j = FP_j - FP_j+1 is the negative class's cell j + 1): 101 products of two
//       converted integers added in order and one division by fl(2 fl(P N_neg)) carry less than 128 roundings, 128 u on a value
//       of at most 1.  The inputs: sum_j |dm_j| <= B_neg with TP_j + TP_j+1 <= 2 P (1 + B_pos), and |d(TP_j + TP_j+1)| <= 2 B_pos
//       with sum_j m_j <= N_neg (1 + B_neg), so |dAUC| <= (B_neg / N_neg + B_pos / P)(1 + B) in units of 1:
//       bound = 1.01 (B_neg 2^-62 / N_neg + B_pos 2^-62 / P) + 256 u.
//   A value is printed when hg_tie4_between(max(v - bound, 0), v + bound) is false (the exact value is never negative, so "-0.0"
//   is not in question); otherwise the call declines with MC_EVAL_DECLINE_ROUNDING_TIE.  An empty class prints nan.
// wave64; every kernel is new HIP for gfx950.  The host side around the kernels is mc_textfeed.h's.
#include "../mc_textfeed.h"
#include "../mc_decimal.h"
#include "../mc_hypergeom.h"
#include "../mc_rowtext.h"

#include <cstring>

namespace {

constexpr int EV_STAGE = 32 * 1024;          // LDS a workgroup of ke_rows stages its 256 lines in
constexpr int EV_C = HG_BUCKETS;             // c = 0 .. 101 (0 unused)
constexpr int EV_VALS = 203;                 // printed values of a table: 101 tpr, 101 fpr, the AUC
constexpr int EV_ROW_W = 96;                 // room of a line of the file (the longest has 73 bytes)
constexpr int EV_MAX_TABLES = 18;
constexpr unsigned long long EV_NO_DECLINE = ~0ull;
constexpr double EV_2P62 = 4611686018427387904.0;

struct EvHead {                              // device-side result block (copied to the host as it is)
    KpHead kp_d, kp_p;                       // the .diffs text, the positions text
    unsigned long long decline_d, decline_p; // min over the offending lines of line << 8 | reason (~0: none)
    unsigned long long n_not_m, n_unlabelled, n_kept;
    unsigned long long n_active, n_pos_sites;        // slots with N > 0; those of the positive class
    unsigned long long n_expect;
    unsigned long long longest_probe;
    unsigned long long tie, deep;            // an expected value on a tie within its bound; a site of 2^31 rows or more
    unsigned long long largest_bound;        // the bits of the largest bound (a non-negative double: its bits order as it does)
    long long out_bytes;
};

struct EvArgs {
    const char *ptext;                       // the positions text, its lines
    int64_t p_bytes, p_lines, p_nl;
    const long long *p_start;
    uint4 *p_tok;                            // per line: tok[0] offset | length << 16, tok[2] the same, bit 0: tok[3][0] == 'm', bit 1: a key
    unsigned long long *p_hash, *p_val;
    unsigned long long *table;               // the truth table; per slot: last line + 1, N, K
    uint64_t mask, hash_mask;
    unsigned int *s_last, *s_N, *s_K;
    const char *text;                        // the .diffs text, its lines
    int64_t n_bytes, n_lines, n_nl;
    const long long *line_start;
    unsigned long long *read_hist, *site_hist;       // [2][102]
    unsigned int *site_list;
    int64_t n_active;
    unsigned long long *cells;               // [depth][2][102][2]: the high halves' sum, the low halves' sum
    unsigned long long *cell_err, *cell_cnt; // [depth][2]
    int64_t min_depth;
    int n_depths, n_tables;
    int depths[16];
    EvHead *head;
    int32_t *vals;                           // [table][203] ten-thousandths, -1: nan
    uint32_t *counts;                        // [table][2 + 202]: P, N_neg, tp[101], fp[101]
    char *rows;
    long long *row_len, *row_off;
    int64_t n_out_lines;
    char *out;
};

__device__ __forceinline__ bool ev_blank(unsigned c) { return c == ' ' || c == '\t'; }

// 1-18 decimal digits -> the value
__device__ __forceinline__ bool ev_digits(const char *s, int n, unsigned long long *v) {
    if (n < 1 || n > 18) return false;
    unsigned long long a = 0;
    for (int i = 0; i < n; ++i) {
        const unsigned d = (unsigned)(unsigned char)s[i] - '0';
        if (d > 9u) return false;
        a = a * 10u + d;
    }
    *v = a;
    return true;
}

__device__ __forceinline__ uint64_t ev_key_hash(const char *chrom, int nc, unsigned long long v, const char *strand, int ns, uint64_t mask) {
    KeyHash H;
    H.span(chrom, nc); H.sep();
    for (int i = 0; i < 8; ++i) H.put((char)(v >> (8 * i)));
    H.sep();
    H.span(strand, ns);
    return H.done(mask);
}

// #{j in 0 .. 100 : p >= j / 100} for 0 <= p <= 1: a guess, put right by the fp64 comparisons the host makes
__device__ __forceinline__ int ev_bucket(double p) {
    int c = (int)(p * 100.0) + 1;
    c = c < 1 ? 1 : c > 101 ? 101 : c;
    while (c < 101 && p >= (double)c / 100.0) ++c;
    while (c > 1 && !(p >= (double)(c - 1) / 100.0)) --c;
    return c;
}

__global__ __launch_bounds__(256) void ke_truth_parse(EvArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.p_lines) return;
    const int64_t b = A.p_start[li];
    const int64_t e = li < A.p_nl ? (int64_t)A.p_start[li + 1] - 1 : A.p_bytes;
    A.p_tok[li] = make_uint4(0u, 0u, 0u, 0u);
    A.p_hash[li] = 0; A.p_val[li] = 0;
    if (e - b > 65535) { line_flag(&A.head->decline_p, li, MC_EVAL_DECLINE_LONG_LINE); return; }
    const char *t = A.ptext + b;
    const int len = (int)(e - b);
    ByteClass bad;
    int o0 = 0, l0 = 0, o1 = 0, l1 = 0, o2 = 0, l2 = 0, o3 = 0, nt = 0;
    bool in = false;
    for (int i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)t[i];
        bad.see(c);
        const bool blank = ev_blank(c);
        if (!blank && !in) {
            o0 = nt == 0 ? i : o0; o1 = nt == 1 ? i : o1; o2 = nt == 2 ? i : o2; o3 = nt == 3 ? i : o3;
        }
        if (blank && in) {
            l0 = nt == 0 ? i - o0 : l0; l1 = nt == 1 ? i - o1 : l1; l2 = nt == 2 ? i - o2 : l2;
            ++nt;
        }
        in = !blank;
    }
    if (in) {
        l0 = nt == 0 ? len - o0 : l0; l1 = nt == 1 ? len - o1 : l1; l2 = nt == 2 ? len - o2 : l2;
        ++nt;
    }
    if (bad.hi) { line_flag(&A.head->decline_p, li, MC_EVAL_DECLINE_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline_p, li, MC_EVAL_DECLINE_CONTROL); return; }
    if (nt < 2) return;
    if (nt < 4) { line_flag(&A.head->decline_p, li, MC_EVAL_DECLINE_POS_TOKENS); return; }
    unsigned long long v = 0;
    if (!ev_digits(t + o1, l1, &v)) { line_flag(&A.head->decline_p, li, MC_EVAL_DECLINE_POS_NUMBER); return; }
    A.p_hash[li] = ev_key_hash(t + o0, l0, v, t + o2, l2, A.hash_mask);
    A.p_val[li] = v;
    A.p_tok[li] = make_uint4((uint32_t)o0 | ((uint32_t)l0 << 16), (uint32_t)o2 | ((uint32_t)l2 << 16), (t[o3] == 'm' ? 1u : 0u) | 2u, 0u);
}

// is (chrom, v, strand) the key of positions line r
__device__ __forceinline__ bool ev_same_key(const EvArgs &A, int64_t r, uint64_t h, unsigned long long v, const char *chrom, int nc, const char *strand,
                                            int ns) {
    if (A.p_hash[r] != h || A.p_val[r] != v) return false;
    const uint4 k = A.p_tok[r];
    if ((int)(k.x >> 16) != nc || (int)(k.y >> 16) != ns) return false;
    const char *q = A.ptext + A.p_start[r];
    return same_bytes(q + (k.x & 0xffffu), chrom, nc) && same_bytes(q + (k.y & 0xffffu), strand, ns);
}

__global__ __launch_bounds__(256) void ke_truth_insert(EvArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.p_lines) return;
    const uint4 k = A.p_tok[li];
    if (!(k.z & 2u)) return;
    const char *t = A.ptext + A.p_start[li];
    const uint64_t h = A.p_hash[li];
    const unsigned long long v = A.p_val[li];
    const KtHit hit = kt_claim(A.table, A.mask, h, li, [&](int64_t r) {
        return ev_same_key(A, r, h, v, t + (k.x & 0xffffu), (int)(k.x >> 16), t + (k.y & 0xffffu), (int)(k.y >> 16));
    });
    if (hit.slot < 0) { line_flag(&A.head->decline_p, li, MC_EVAL_DECLINE_TABLE); return; }
    atomicMax(&A.s_last[hit.slot], (unsigned int)(li + 1));
}

// one .diffs line, in the host's order.  s_cnt: not M, unlabelled, kept
__device__ __forceinline__ void ev_row(const EvArgs &A, const char *t, int64_t adj, int64_t li, unsigned int *s_hist, unsigned int *s_cnt) {
    const int64_t b = A.line_start[li];
    const int64_t e = li < A.n_nl ? (int64_t)A.line_start[li + 1] - 1 : A.n_bytes;
    if (e - b > 65535) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_LONG_LINE); return; }
    const char *q = t + (b - adj);
    const int len = (int)(e - b);
    ByteClass bad;
    int t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0, nt = 0;
    for (int i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)q[i];
        bad.see(c);
        if (c == '\t') {
            t0 = nt == 0 ? i : t0; t1 = nt == 1 ? i : t1; t2 = nt == 2 ? i : t2; t3 = nt == 3 ? i : t3;
            t4 = nt == 4 ? i : t4; t5 = nt == 5 ? i : t5; t6 = nt == 6 ? i : t6;
            ++nt;
        }
    }
    if (bad.hi) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_CONTROL); return; }
    if (nt != 7) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_FIELDS); return; }
    const int cl = t3 - t2 - 1;
    if (cl == 0) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_CONTEXT); return; }
    if (q[t2 + 1 + cl / 2] != 'M') { atomicAdd(&s_cnt[0], 1u); return; }
    unsigned long long v = 0;
    if (!ev_digits(q + t1 + 1, t2 - t1 - 1, &v)) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_POSITION); return; }
    const char *strand = q + t4 + 1;
    const int ns = t5 - t4 - 1;
    const uint64_t h = ev_key_hash(q, t0, v, strand, ns, A.hash_mask);
    const KtHit hit = kt_find(A.table, A.mask, h, [&](int64_t r) { return ev_same_key(A, r, h, v, q, t0, strand, ns); });
    if (hit.looked > A.head->longest_probe) atomicMax(&A.head->longest_probe, (unsigned long long)hit.looked);
    if (hit.slot < 0) { atomicAdd(&s_cnt[1], 1u); return; }
    int pb = t6 + 1, pe = len;
    while (pb < pe && q[pb] == ' ') ++pb;
    while (pe > pb && q[pe - 1] == ' ') --pe;
    double p = 0.0;
    if (!dc_parse(q + pb, pe - pb, &p) || !(p >= 0.0 && p <= 1.0)) { line_flag(&A.head->decline_d, li, MC_EVAL_DECLINE_PROBABILITY); return; }
    atomicAdd(&s_cnt[2], 1u);
    atomicAdd(&A.s_N[hit.slot], 1u);
    if (t6 - t5 - 1 > 0 && q[t5 + 1] == 'm') atomicAdd(&A.s_K[hit.slot], 1u);
    const unsigned cls = A.p_tok[A.s_last[hit.slot] - 1].z & 1u;
    atomicAdd(&s_hist[cls * EV_C + ev_bucket(p)], 1u);
}

__global__ __launch_bounds__(256) void ke_rows(EvArgs A) {
    __shared__ unsigned int s_hist[2 * EV_C], s_cnt[3];
    if (threadIdx.x < 2 * EV_C) s_hist[threadIdx.x] = 0u;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    (void)staged_lines<EV_STAGE>(A.text, A.n_bytes, A.line_start, A.n_lines, A.n_nl,
                                 [&](const char *t, int64_t adj, int64_t li) { ev_row(A, t, adj, li, s_hist, s_cnt); });
    __syncthreads();
    if (threadIdx.x < 2 * EV_C && s_hist[threadIdx.x]) atomicAdd(&A.read_hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
    if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&A.head->n_not_m, (unsigned long long)s_cnt[0]);
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&A.head->n_unlabelled, (unsigned long long)s_cnt[1]);
    if (threadIdx.x == 2 && s_cnt[2]) atomicAdd(&A.head->n_kept, (unsigned long long)s_cnt[2]);
}

__global__ __launch_bounds__(256) void ke_sites(EvArgs A) {
    const uint64_t slot = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot > A.mask || A.table[slot] == 0ull) return;
    const unsigned int N = A.s_N[slot], K = A.s_K[slot];
    if (N == 0u) return;
    if (N >= 0x80000000u) { A.head->deep = 1ull; return; }
    const unsigned cls = A.p_tok[A.s_last[slot] - 1].z & 1u;
    const unsigned long long at = atomicAdd(&A.head->n_active, 1ull);
    if (at <= A.mask) A.site_list[at] = (unsigned int)slot;              // (as many entries of room as slots)
    if (cls) atomicAdd(&A.head->n_pos_sites, 1ull);
    if ((int64_t)N >= A.min_depth) atomicAdd(&A.site_hist[cls * EV_C + ev_bucket((double)K / (double)N)], 1ull);
}

struct EvCellSink {
    unsigned long long *cell;                // the class's [102][2] in LDS
    unsigned int n_put;
    __device__ __forceinline__ void put(int c, double v) {
        const unsigned long long q = (unsigned long long)(v * EV_2P62);
        atomicAdd(&cell[2 * c], q >> 32);
        atomicAdd(&cell[2 * c + 1], q & 0xffffffffull);
        ++n_put;
    }
};

__global__ __launch_bounds__(256) void ke_expect(EvArgs A) {
    __shared__ unsigned long long s_cell[2 * EV_C * 2], s_err[2], s_n[2];
    for (int i = threadIdx.x; i < 2 * EV_C * 2; i += 256) s_cell[i] = 0ull;
    if (threadIdx.x < 2) { s_err[threadIdx.x] = 0ull; s_n[threadIdx.x] = 0ull; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int di = (int)blockIdx.y;
    const int64_t d = A.depths[di];
    if (i < A.n_active) {
        const unsigned int slot = A.site_list[i];
        const int64_t N = A.s_N[slot], K = A.s_K[slot];
        if (N >= d) {
            const unsigned cls = A.p_tok[A.s_last[slot] - 1].z & 1u;
            EvCellSink sink = {s_cell + cls * EV_C * 2, 0u};
            double err = 0.0;
            (void)hg_masses_to(N, K, d, sink, &err);
            atomicAdd(&s_n[cls], 1ull);
            if (!(err < 4.656612873077393e-10)) A.head->tie = 1ull;      // (2^-31: no such bound; nothing is printed from it)
            else if (err > 0.0) atomicAdd(&s_err[cls], (unsigned long long)ceil(err * EV_2P62) + sink.n_put);
        }
    }
    __syncthreads();
    unsigned long long *cells = A.cells + (size_t)di * 2 * EV_C * 2;
    for (int k = threadIdx.x; k < 2 * EV_C * 2; k += 256)
        if (s_cell[k]) atomicAdd(&cells[k], s_cell[k]);
    if (threadIdx.x < 2) {
        if (s_err[threadIdx.x]) atomicAdd(&A.cell_err[di * 2 + threadIdx.x], s_err[threadIdx.x]);
        if (s_n[threadIdx.x]) {
            atomicAdd(&A.cell_cnt[di * 2 + threadIdx.x], s_n[threadIdx.x]);
            atomicAdd(&A.head->n_expect, s_n[threadIdx.x]);
        }
    }
}

// a / b correctly rounded (half-way to even): Python's int / int.  0 <= a, 0 < b < 2^63, a <= 2 b
__device__ __forceinline__ double ev_quot(unsigned long long a, unsigned long long b) {
    if (a == 0ull) return 0.0;
    const int s = dc_clz64(a);
    const uint64_t n1 = a << s;                                          // (n1 : 0) = a << (s + 64)
    const uint64_t qh = n1 / b;
    uint64_t rem;
    const uint64_t ql = dc_div128(n1 - qh * b, 0ull, b, &rem);
    const uint64_t bits = dc_round(qh, ql, rem != 0, -s - 64);
    double v;
    __builtin_memcpy(&v, &bits, 8);
    return v;
}

// an integer below 2^104 as a double: one rounding
__device__ __forceinline__ double ev_to_double(unsigned __int128 x) {
    return (double)(unsigned long long)(x >> 52) * 4503599627370496.0 + (double)(unsigned long long)(x & (((unsigned __int128)1 << 52) - 1));
}

__device__ __forceinline__ unsigned __int128 ev_cell(const unsigned long long *cc, int cls, int c) {
    return ((unsigned __int128)cc[(cls * EV_C + c) * 2] << 32) + cc[(cls * EV_C + c) * 2 + 1];
}

__device__ __forceinline__ void ev_bound_seen(EvHead *head, double v, double bound) {
    const double lo = v - bound > 0.0 ? v - bound : 0.0;
    if (hg_tie4_between(lo, v + bound)) head->tie = 1ull;
    unsigned long long bits;
    __builtin_memcpy(&bits, &bound, 8);
    if (bits > head->largest_bound) atomicMax(&head->largest_bound, bits);
}

// the AUC of an integer table: tp / fp as per-bucket counts h[cls * 102 + c]
__device__ __forceinline__ double ev_int_auc(const unsigned long long *neg, const unsigned long long *pos, int stride, int shift, unsigned long long P,
                                             unsigned long long Nn) {
    unsigned long long A = 0, tp_next = 0;
    for (int j = 100; j >= 0; --j) {
        const unsigned long long tp = tp_next + (pos[(j + 1) * stride] >> shift);
        A += (neg[(j + 1) * stride] >> shift) * (tp + tp_next);
        tp_next = tp;
    }
    return ev_quot(A, 2ull * P * Nn);
}

__global__ __launch_bounds__(256) void ke_finish(EvArgs A) {
    const int t = (int)blockIdx.x, v = (int)threadIdx.x;
    if (v >= EV_VALS) return;
    const double nan = __builtin_nan("");
    const double u = 1.1102230246251565e-16;
    double val = nan;
    uint32_t *counts = A.counts + (size_t)t * (2 + 202);
    if (t < 2) {
        const unsigned long long *h = t == 0 ? A.read_hist : A.site_hist;
        unsigned long long P = 0, Nn = 0;
        for (int c = 1; c < EV_C; ++c) { P += h[EV_C + c]; Nn += h[c]; }
        if (v < 202) {
            const int cls = v < 101 ? 1 : 0, j = v < 101 ? v : v - 101;
            unsigned long long s = 0;
            for (int c = j + 1; c < EV_C; ++c) s += h[cls * EV_C + c];
            const unsigned long long n = cls ? P : Nn;
            if (n) val = ev_quot(s, n);
            counts[2 + v] = (uint32_t)s;
        } else {
            counts[0] = (uint32_t)P; counts[1] = (uint32_t)Nn;
            if (P && Nn) val = ev_int_auc(h, h + EV_C, 1, 0, P, Nn);
        }
    } else {
        const int di = t - 2;
        const unsigned long long *cc = A.cells + (size_t)di * 2 * EV_C * 2;
        const unsigned long long P = A.cell_cnt[di * 2 + 1], Nn = A.cell_cnt[di * 2];
        const unsigned long long Bp = A.cell_err[di * 2 + 1], Bn = A.cell_err[di * 2];
        if (v < 202) {
            const int cls = v < 101 ? 1 : 0, j = v < 101 ? v : v - 101;
            const unsigned long long n = cls ? P : Nn, B = cls ? Bp : Bn;
            unsigned __int128 E = 0;
            for (int c = j + 1; c < EV_C; ++c) E += ev_cell(cc, cls, c);
            if (n && B == 0ull) val = ev_quot((unsigned long long)(E >> 62), n);
            else if (n) {
                val = ev_to_double(E) / EV_2P62 / (double)n;
                ev_bound_seen(A.head, val, 1.0000001 * ((double)B / EV_2P62 / (double)n) + 8.0 * u * val);
            }
            counts[2 + v] = 0u;
        } else {
            counts[0] = (uint32_t)P; counts[1] = (uint32_t)Nn;
            if (P && Nn && Bp == 0ull && Bn == 0ull) {
                // (every cell is a count << 62: its high-halves' sum is the count << 30, its low-halves' sum 0)
                val = ev_int_auc(cc, cc + EV_C * 2, 2, 30, P, Nn);
            } else if (P && Nn) {
                double sum = 0.0;
                unsigned __int128 tp_next = 0;
                for (int j = 100; j >= 0; --j) {
                    const unsigned __int128 tp = tp_next + ev_cell(cc, 1, j + 1);
                    sum += ev_to_double(ev_cell(cc, 0, j + 1)) * ev_to_double(tp + tp_next);
                    tp_next = tp;
                }
                val = sum / EV_2P62 / EV_2P62 / (2.0 * ((double)P * (double)Nn));
                ev_bound_seen(A.head, val, 1.01 * ((double)Bn / EV_2P62 / (double)Nn + (double)Bp / EV_2P62 / (double)P) + 256.0 * u);
            }
        }
    }
    A.vals[t * EV_VALS + v] = val == val ? (int32_t)rint(val * 10000.0) : -1;
}

__device__ __forceinline__ void ev_put_text(RtStore &o, const char *s) { for (; *s; ++s) o.put(*s); }

__device__ __forceinline__ void ev_put_val(RtStore &o, int32_t r) {
    if (r < 0) ev_put_text(o, "nan");
    else rt_put_fixed4(o, r);
}

__device__ __forceinline__ void ev_put_table(RtStore &o, const EvArgs &A, int t) {
    if (t == 0) ev_put_text(o, "read\t-");
    else if (t == 1) ev_put_text(o, "site\tall");
    else { ev_put_text(o, "site\t"); rt_put_uint(o, (uint32_t)A.depths[t - 2]); }
}

__global__ __launch_bounds__(256) void ke_write(EvArgs A) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= A.n_out_lines) return;
    char *start = A.rows + l * EV_ROW_W;
    RtStore o = {start};
    const int n_rows = A.n_tables * 101;
    if (l == 0) {
        ev_put_text(o, "#level\tdepth\tthreshold\tn_pos\tn_neg\ttp\tfp\ttpr\tfpr");
    } else if (l <= n_rows) {
        const int t = (int)(l - 1) / 101, j = (int)(l - 1) % 101;
        const uint32_t *counts = A.counts + (size_t)t * (2 + 202);
        ev_put_table(o, A, t); o.put('\t');
        rt_put_fixed4(o, j * 100); o.put('\t');                         // repr(j / 100)
        rt_put_uint(o, counts[0]); o.put('\t');
        rt_put_uint(o, counts[1]); o.put('\t');
        if (t < 2) { rt_put_uint(o, counts[2 + j]); o.put('\t'); rt_put_uint(o, counts[2 + 101 + j]); }
        else { o.put('-'); o.put('\t'); o.put('-'); }
        o.put('\t');
        ev_put_val(o, A.vals[t * EV_VALS + j]); o.put('\t');
        ev_put_val(o, A.vals[t * EV_VALS + 101 + j]);
    } else {
        const int t = (int)(l - 1 - n_rows);
        ev_put_text(o, "auc\t");
        ev_put_table(o, A, t); o.put('\t');
        ev_put_val(o, A.vals[t * EV_VALS + 202]);
    }
    o.put('\n');
    A.row_len[l] = (long long)(o.p - start);
}

__global__ __launch_bounds__(256) void ke_pack(EvArgs A) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= A.n_out_lines) return;
    const long long at = A.row_off[l], n = A.row_len[l];
    if (at < 0 || n > EV_ROW_W || at + n > A.n_out_lines * EV_ROW_W) return;       // (cannot be: the scan counted these bytes)
    const char *src = A.rows + l * EV_ROW_W;
    for (long long i = 0; i < n; ++i) A.out[at + i] = src[i];
}

const char *ev_reason_text(int reason) {
    switch (reason) {
    case MC_EVAL_DECLINE_HIGH_BYTE: return "a byte >= 0x80";
    case MC_EVAL_DECLINE_CONTROL: return "a control byte";
    case MC_EVAL_DECLINE_LONG_LINE: return "a line of more than 65535 bytes";
    case MC_EVAL_DECLINE_FIELDS: return "a line that is not eight tab-separated fields";
    case MC_EVAL_DECLINE_CONTEXT: return "an empty context";
    case MC_EVAL_DECLINE_POSITION: return "a position that is not 1-18 decimal digits";
    case MC_EVAL_DECLINE_PROBABILITY: return "a probability that is no plain decimal inside [0, 1]";
    case MC_EVAL_DECLINE_POS_TOKENS: return "a positions line of fewer than four tokens";
    case MC_EVAL_DECLINE_POS_NUMBER: return "a positions line whose second token is not 1-18 decimal digits";
    case MC_EVAL_DECLINE_TABLE: return "the truth table is full";
    case MC_EVAL_DECLINE_MEMORY: return "the texts do not fit into free device memory beside their tables";
    case MC_EVAL_DECLINE_ROWS: return "2^31 - 2 lines or more";
    case MC_EVAL_DECLINE_DEPTH: return "a site of 2^31 rows or more";
    case MC_EVAL_DECLINE_ROUNDING_TIE: return "an expected value within its bound of a tie of np.round(., 4)";
    }
    return "?";
}

int ev_decline(mc_ctx *c, int32_t *status, int reason, long long line, int file) {
    c->eval.stats.decline_file = file;
    return decline(c->eval.stats, status, file ? "evaluation (the positions file)" : "evaluation", ev_reason_text(reason), reason, line);
}

// MCALLER_EVAL_DEVICE_BYTES=n stands for the free device memory (tests)
bool ev_fits(size_t bytes) { return fits("MCALLER_EVAL_DEVICE_BYTES", bytes); }

inline unsigned ev_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// both texts are on the device (padded): everything behind that
int ev_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const char *d_ptext, int64_t np, const mc_eval_params *P, const char **out,
           int64_t *n_out, int32_t *status) {
    mc_eval_stats &S = c->eval.stats;
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    auto t_step = std::chrono::steady_clock::now();
    EvHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline_d = h.decline_p = EV_NO_DECLINE;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    EvArgs A = {};
    A.head = d_head;
    A.ptext = d_ptext; A.p_bytes = np;
    A.text = d_text; A.n_bytes = n;
    A.min_depth = P->min_depth; A.n_depths = P->n_depths; A.n_tables = 2 + P->n_depths;
    for (int i = 0; i < P->n_depths; ++i) A.depths[i] = P->depths[i];
    const char *hm = getenv("MCALLER_EVAL_HASH_MASK");
    A.hash_mask = hm && *hm ? strtoull(hm, nullptr, 16) : ~0ull;       // (tests: long probe chains)
    size_t held = (size_t)n + (size_t)np + 128;

    // ---- the truth ----
    long long *tile_off = nullptr, *p_start = nullptr;
    if (np > 0) {
        if (int rc = lines_count(pool, st, d_ptext, np, &d_head->kp_p, &tile_off)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (too_many_lines(h.kp_p.n_newlines)) return ev_decline(c, status, MC_EVAL_DECLINE_ROWS, -1, 1);
        if (!ev_fits(held + (size_t)(h.kp_p.n_newlines + 2) * (8 + 32 + 2 * 20) + ((size_t)1 << 20))) return ev_decline(c, status, MC_EVAL_DECLINE_MEMORY, -1, 1);
        if (int rc = lines_starts(pool, st, d_ptext, np, h.kp_p.n_newlines, tile_off, &d_head->kp_p, &p_start)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        A.p_lines = h.kp_p.n_lines; A.p_nl = h.kp_p.n_newlines; A.p_start = p_start;
    }
    S.n_pos_lines = A.p_lines;
    const size_t pl = (size_t)std::max<int64_t>(A.p_lines, 1);
    const uint64_t slots = table_slots(A.p_lines, 1024, "MCALLER_EVAL_TABLE_SLOTS");
    A.mask = slots - 1;
    S.table_slots = (int64_t)slots;
    if (pool.get(&A.p_tok, pl) || pool.get(&A.p_hash, pl) || pool.get(&A.p_val, pl) || pool.get(&A.s_last, (size_t)slots) ||
        pool.get(&A.s_N, (size_t)slots) || pool.get(&A.s_K, (size_t)slots) || pool.get(&A.site_list, (size_t)slots))
        return -10;
    if (int rc = table_get(pool, st, &A.table, slots)) return rc;
    held += pl * 32 + (size_t)slots * 24 + (size_t)(A.p_lines + 2) * 8;
    HIP_TRY(hipMemsetAsync(A.s_last, 0, (size_t)slots * 4, st));
    HIP_TRY(hipMemsetAsync(A.s_N, 0, (size_t)slots * 4, st));
    HIP_TRY(hipMemsetAsync(A.s_K, 0, (size_t)slots * 4, st));
    const size_t n_hist = 2 * EV_C, n_cells = (size_t)std::max(A.n_depths, 1) * 2 * EV_C * 2, n_dc = (size_t)std::max(A.n_depths, 1) * 2;
    if (pool.get(&A.read_hist, n_hist) || pool.get(&A.site_hist, n_hist) || pool.get(&A.cells, n_cells) || pool.get(&A.cell_err, n_dc) ||
        pool.get(&A.cell_cnt, n_dc))
        return -10;
    HIP_TRY(hipMemsetAsync(A.read_hist, 0, n_hist * 8, st));
    HIP_TRY(hipMemsetAsync(A.site_hist, 0, n_hist * 8, st));
    HIP_TRY(hipMemsetAsync(A.cells, 0, n_cells * 8, st));
    HIP_TRY(hipMemsetAsync(A.cell_err, 0, n_dc * 8, st));
    HIP_TRY(hipMemsetAsync(A.cell_cnt, 0, n_dc * 8, st));
    if (A.p_lines > 0) {
        hipLaunchKernelGGL(ke_truth_parse, dim3(ev_blocks(A.p_lines)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(ke_truth_insert, dim3(ev_blocks(A.p_lines)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.decline_p != EV_NO_DECLINE) return ev_decline(c, status, decline_reason(h.decline_p), decline_line(h.decline_p), 1);
    S.ms_truth = ms_since(t_step);
    t_step = std::chrono::steady_clock::now();

    // ---- the rows, the sites ----
    long long *line_start = nullptr;
    if (n > 0) {
        if (int rc = lines_count(pool, st, d_text, n, &d_head->kp_d, &tile_off)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (too_many_lines(h.kp_d.n_newlines)) return ev_decline(c, status, MC_EVAL_DECLINE_ROWS, -1, 0);
        if (!ev_fits(held + (size_t)(h.kp_d.n_newlines + 2) * 8 + ((size_t)1 << 20))) return ev_decline(c, status, MC_EVAL_DECLINE_MEMORY, -1, 0);
        if (int rc = lines_starts(pool, st, d_text, n, h.kp_d.n_newlines, tile_off, &d_head->kp_d, &line_start)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        A.n_lines = h.kp_d.n_lines; A.n_nl = h.kp_d.n_newlines; A.line_start = line_start;
        held += (size_t)(A.n_lines + 2) * 8;
        if (A.n_lines > 0) hipLaunchKernelGGL(ke_rows, dim3(ev_blocks(A.n_lines)), dim3(256), EV_STAGE + 16, st, A);
    }
    S.n_rows = A.n_lines;
    hipLaunchKernelGGL(ke_sites, dim3(ev_blocks((int64_t)slots)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.decline_d != EV_NO_DECLINE) return ev_decline(c, status, decline_reason(h.decline_d), decline_line(h.decline_d), 0);
    if (h.deep) return ev_decline(c, status, MC_EVAL_DECLINE_DEPTH, -1, 0);
    S.n_kept = (int64_t)h.n_kept; S.n_unlabelled = (int64_t)h.n_unlabelled; S.n_not_m = (int64_t)h.n_not_m;
    S.n_sites = (int64_t)h.n_active; S.n_pos_sites = (int64_t)h.n_pos_sites; S.n_neg_sites = S.n_sites - S.n_pos_sites;
    S.longest_probe = (int64_t)h.longest_probe;
    S.ms_rows = ms_since(t_step);
    t_step = std::chrono::steady_clock::now();

    // ---- the expectation over the draws ----
    A.n_active = (int64_t)std::min<unsigned long long>(h.n_active, slots);
    if (A.n_active > 0 && A.n_depths > 0) {
        hipLaunchKernelGGL(ke_expect, dim3(ev_blocks(A.n_active), (unsigned)A.n_depths), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    S.ms_expect = ms_since(t_step);
    t_step = std::chrono::steady_clock::now();

    // ---- the values, the file ----
    A.n_out_lines = 1 + (int64_t)A.n_tables * 102;
    const size_t nl = (size_t)A.n_out_lines;
    if (pool.get(&A.vals, (size_t)A.n_tables * EV_VALS) || pool.get(&A.counts, (size_t)A.n_tables * (2 + 202)) || pool.get(&A.rows, nl * EV_ROW_W) ||
        pool.get(&A.row_len, nl) || pool.get(&A.row_off, nl) || pool.get(&A.out, nl * EV_ROW_W))
        return -10;
    held += nl * (2 * EV_ROW_W + 16) + (size_t)A.n_tables * 2048 + (size_t)(n_hist * 2 + n_cells + 2 * n_dc) * 8;
    S.kernel_bytes = (int64_t)held;
    hipLaunchKernelGGL(ke_finish, dim3((unsigned)A.n_tables), dim3(256), 0, st, A);
    hipLaunchKernelGGL(ke_write, dim3(ev_blocks(A.n_out_lines)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.row_len, A.n_out_lines, A.row_off, &d_head->out_bytes);
    hipLaunchKernelGGL(ke_pack, dim3(ev_blocks(A.n_out_lines)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_expect = (int64_t)h.n_expect;
    __builtin_memcpy(&S.largest_bound, &h.largest_bound, 8);
    if (h.tie) return ev_decline(c, status, MC_EVAL_DECLINE_ROUNDING_TIE, -1, 0);
    S.ms_finish = ms_since(t_step);
    t_step = std::chrono::steady_clock::now();
    if (h.out_bytes < 0 || (size_t)h.out_bytes > nl * EV_ROW_W) { mc_set_error("mc_eval_calls: the file's size is off"); return -1; }
    if (int rc = fetch_out(c, c->eval.out, A.out, (size_t)h.out_bytes, out, n_out)) return rc;
    S.ms_d2h = ms_since(t_step);
    return 0;
}

int ev_call(mc_ctx *c, const mc_text_source &src, const mc_text_source &pos, const mc_eval_params *P, const char **out, int64_t *n_out, int32_t *status) {
    mc_eval_stats &S = c->eval.stats;
    return pipeline_call(c, S, status, "evaluation", (size_t)64 << 20, [&] { *out = nullptr; *n_out = 0; }, [&](Call &K) -> int {
        S.n_bytes = src.n_bytes;
        S.n_pos_bytes = pos.n_bytes;
        if (!ev_fits((size_t)src.n_bytes + (size_t)pos.n_bytes + ((size_t)1 << 20))) return ev_decline(c, status, MC_EVAL_DECLINE_MEMORY, -1, 0);
        char *d_text = nullptr, *d_ptext = nullptr;
        if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;
        if (int rc = K.feed.put(K.pool, pos, &d_ptext)) return rc;
        K.feed.times(S, K.t0);
        return ev_run(c, K.pool, d_text, src.n_bytes, d_ptext, pos.n_bytes, P, out, n_out, status);
    });
}

struct HgMassOut {
    double *mass;
    __device__ __forceinline__ void put(int c, double v) { mass[c] = v; }
};

// the probe of hg_masses' device build: a lane per case, the masses straight into the lane's 102 doubles (bad arguments: NaN everywhere)
__global__ __launch_bounds__(256) void k_hg_masses_probe(const long long *__restrict__ N, const long long *__restrict__ K, const long long *__restrict__ d,
                                                         int64_t count, double *__restrict__ mass, double *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double *m = mass + i * HG_BUCKETS;
    for (int c = 0; c < HG_BUCKETS; ++c) m[c] = 0.0;
    HgMassOut sink = {m};
    double e;
    if (hg_masses_to(N[i], K[i], d[i], sink, &e) != HG_OK)
        for (int c = 0; c < HG_BUCKETS; ++c) m[c] = __builtin_nan("");
    err[i] = e;
}

}  // namespace

extern "C" int mc_eval_calls(mc_ctx *c, const mc_text_source *diffs, const mc_text_source *positions, const mc_eval_params *P, const char **out,
                             int64_t *n_out, int32_t *status) {
    bool ok = c && P && out && n_out && status && P->n_depths >= 0 && P->n_depths <= 16;
    for (int i = 0; ok && i < P->n_depths; ++i) ok = P->depths[i] >= 1 && P->depths[i] <= 1024 && (i == 0 || P->depths[i] > P->depths[i - 1]);
    if (!ok) {
        mc_set_error("mc_eval_calls: bad arguments");
        return -12;
    }
    mc_text_source s = {}, p = {};
    if (int rc = text_source("mc_eval_calls", diffs, &s)) return rc;
    if (int rc = text_source("mc_eval_calls", positions, &p)) return rc;
    return ev_call(c, s, p, P, out, n_out, status);
}

extern "C" int mc_eval_last_stats(mc_ctx *c, mc_eval_stats *out) { return stats_out("mc_eval_last_stats", c, out, &mc_ctx::eval, &EvalPipe::stats); }

extern "C" int mc_eval_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::eval); }

extern "C" int mc_hypergeom_masses_device(mc_ctx *c, const int64_t *N, const int64_t *K, const int64_t *d, int64_t count, double *mass102, double *err) {
    if (!c || count < 0 || (count > 0 && (!N || !K || !d || !mass102 || !err))) {
        mc_set_error("mc_hypergeom_masses_device: bad arguments");
        return -12;
    }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Pool pool("hypergeometric masses probe");
    long long *d_in = nullptr;
    double *d_out = nullptr;
    if (pool.get(&d_in, (size_t)count * 3) || pool.get(&d_out, (size_t)count * (HG_BUCKETS + 1))) return -10;
    hipStream_t st = c->stream;
    const int64_t *in[3] = {N, K, d};
    for (int q = 0; q < 3; ++q) HIP_TRY(hipMemcpyAsync(d_in + q * count, in[q], (size_t)count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hg_masses_probe, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const long long *)d_in, (const long long *)(d_in + count),
                       (const long long *)(d_in + 2 * count), count, d_out, d_out + count * HG_BUCKETS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mass102, d_out, (size_t)count * HG_BUCKETS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(err, d_out + count * HG_BUCKETS, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
