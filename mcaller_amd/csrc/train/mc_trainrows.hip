// mc_trainrows.hip -- the rows of a `--training_tsv` file (`.diffs.<k>.train`) as matrices, made on the GPU: what
// load_mCaller_data.py:14-29 (tsv2matrix) builds line by line in Python (C ABI: mc_train_rows, mc_train_rows_last_stats,
// mc_train_rows_release; Python: Device.training_rows, load_mCaller_data.tsv2matrix_device).  The unit stands in csrc/train/, beside
// the units of the passes like csrc/bed/: no pass runs its kernels.  mc_parse_doubles_device, the probe of mc_decimal.h's device
// build (Device.parse_doubles), lives here too: this unit is that header's device user.
//
// A row: tab-separated fields, field 3 the context, field 4 the comma-separated features, field 6 the label (stripped; 7 fields or
// more: a predict-mode row carries its probability behind the label).  A label is registered by the first row that carries it; a
// row is kept iff it has >= 6 features and none is the literal "0"; kept rows go to their label's matrix in file order, labels in
// first-occurrence order.  Every number is mc_decimal.h's correctly rounded double, or the call declines and the host code does
// the file (status 1, mc_last_error; MC_TRAINROWS_DECLINE_*):
//   * a byte >= 0x80; a control byte other than tab and newline (0x7f too; '\r': Python's universal newlines split there)
//   * a line with fewer than 7 tab-separated fields (the empty line is one: the host raises there as the reference does)
//   * a context whose centre pair context[len/2 : len/2 + 2] is not among the accepted pairs (the host raises its KeyError)
//   * a kept row with a number mc_decimal.h declines (a left-out row's numbers are never looked at)
//   * kept rows with differing feature counts, or a kept row with more than 64 features
//   * a context longer than 63 bytes
//   * more than 16 distinct labels
//   * a line longer than 65535 bytes (offsets inside a line are 16 bits; a long line within that is read in place, not staged)
//   * 2^31 - 2 lines or more (a slot of the label table holds row + 1 in 32 bits)
//   * a text that does not fit into free device memory beside its outputs: the WHOLE text stays resident
//
// The steps (one lane per line unless said otherwise; n = lines):
//   kp_count / kp_scan / kp_starts   line starts (the device parser's kernels: mc_lines.h, launched by mc_textfeed.h)
//   kt_parse     256 lines of a workgroup through LDS (staged_lines, mc_textdev.h; a piece that does not fit: read in place, and
//                counted); per line the class of every byte, the tabs, the context's span and centre pair, the stripped label's
//                span and the KeyHash of its bytes, the commas of the feature field, the literal-"0" test, the kept flag.  A
//                flagged line: line_flag; the first kept line's feature count by an atomicMin of the same form
//   kt_intern    labels into the key table of 64 slots inside the head (kt_claim; ids are rows); atomicMin of the line per slot.
//                The host orders the (at most 16) taken slots by that line: label ids do not depend on the order of arrival
//   kt_count / kp_scan / kt_rank   kept rows per label and workgroup, exclusive scan label-major: a kept row's place among all
//                rows of the result (ballots and scans, never atomicAdd: file order is part of the contract); kt_rank also
//                lists the row's feature tokens (offset | length << 16) and checks its feature count
//   kt_place     a lane per NUMBER: mc_decimal.h on the token -> X[row][j]; lane j = 0 copies the context, NUL-padded
// wave64; no library sort; every buffer, event and stream through the owners of mc_own.h.
// The host side around the kernels -- a file's way onto the device through the context's two pinned stages, the line starts, the
// head's way back, the decline, the clock -- is mc_textfeed.h's, the device side named above mc_textdev.h's: shared with the other
// units that take a whole text file.
#include "../mc_textfeed.h"
#include "../mc_decimal.h"

#include <cstring>

namespace {

constexpr int TR_STAGE = 48 * 1024;          // LDS a workgroup of kt_parse stages its 256 lines in
constexpr int TR_SLOTS = 64;                 // slots of the label table (a power of two, four times the labels a file may have)
constexpr unsigned TR_F_KEPT = 1;

struct TrHead {                              // device-side result block (copied to the host as it is)
    KpHead kp;                               // n_newlines (kp_scan), n_lines (kp_starts)
    unsigned long long decline;              // min over the flagged lines of line << 8 | reason (~0: none)
    unsigned long long first_kept;           // min over the kept lines of line << 8 | features (~0: none)
    unsigned long long table[TR_SLOTS];      // the labels' key table (mc_textdev.h; ids are rows)
    unsigned long long first[TR_SLOTS];      // the smallest line that carries the slot's label
    long long n_kept;                        // total of the scan
    unsigned int n_claimed;                  // slots taken (+ 1000 for every row that found the table full)
    unsigned int in_place;                   // workgroups of kt_parse that read their lines in place
    int max_ctx, pad;
    // what the host sends down
    uint16_t pairs[MC_TRAINROWS_MAX_PAIRS];
    uint8_t id_of_slot[TR_SLOTS];
};

struct TrArgs {
    const char *text;
    int64_t n_bytes, n_lines, n_nl;
    const long long *line_start;
    TrHead *head;
    // per line: x = feature field begin | end << 16, y = context begin | length << 16, z = label begin | length << 16, w = features | flags << 16
    uint4 *row;
    uint64_t *hash;
    uint8_t *slot;
    uint64_t hash_mask;
    int n_pairs, n_labels, nf, ctx_w;
    long long *blk_cnt, *blk_off;            // [n_labels * nblk] each, label-major
    int64_t nblk, n_kept;
    // per kept row, in the order of the result
    uint32_t *row_line, *tok;                // tok: [n_kept * nf]
    double *X;
    char *ctx;
};

// One line: t[x - adj] is byte x of the text (the staged piece in LDS, or the text itself with adj = 0: one address space per call
// site) -> the context's length if the row is kept, -1 if it is not
__device__ __forceinline__ int tr_parse_line(const TrArgs &A, const char *t, const int64_t adj, const int64_t li) {
    const int64_t b = A.line_start[li] - adj;
    const int64_t e = (li < A.n_nl ? A.line_start[li + 1] - 1 : A.n_bytes) - adj;        // the newline, or the end of the text
    A.row[li] = make_uint4(0u, 0u, 0u, 0u);
    A.hash[li] = 0;
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_TRAINROWS_DECLINE_LONG_LINE); return -1; }
    const int len = (int)(e - b);
    int t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0, nt = 0;
    ByteClass bad;
    bool has0 = false;
    int commas = 0, flen = 0;
    unsigned lastc = 0;
    for (int i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)t[b + i];
        bad.see(c);
        if (c == '\t') {
            t2 = nt == 2 ? i : t2; t3 = nt == 3 ? i : t3; t4 = nt == 4 ? i : t4; t5 = nt == 5 ? i : t5; t6 = nt == 6 ? i : t6;
            ++nt;
        } else if (nt == 4) {                                     // the feature field: its commas, a field that is "0"
            if (c == ',') { has0 |= flen == 1 && lastc == '0'; ++commas; flen = 0; }
            else { ++flen; lastc = c; }
        }
    }
    has0 |= flen == 1 && lastc == '0';
    int reason = 0;
    if (bad.hi) reason = MC_TRAINROWS_DECLINE_HIGH_BYTE;
    else if (bad.ctrl) reason = MC_TRAINROWS_DECLINE_CONTROL;
    else if (nt < 6) reason = MC_TRAINROWS_DECLINE_FIELDS;
    if (reason) { line_flag(&A.head->decline, li, reason); return -1; }
    if (nt == 6) t6 = len;
    const int cb = t2 + 1, cn = t3 - t2 - 1;
    if (cn > MC_TRAINROWS_MAX_CONTEXT) { line_flag(&A.head->decline, li, MC_TRAINROWS_DECLINE_CONTEXT); return -1; }
    bool known = false;
    if (cn / 2 + 2 <= cn) {                                       // (a shorter slice is no two-character key)
        const unsigned pair = (unsigned)(unsigned char)t[b + cb + cn / 2] | ((unsigned)(unsigned char)t[b + cb + cn / 2 + 1] << 8);
        for (int k = 0; k < A.n_pairs; ++k) known |= (unsigned)A.head->pairs[k] == pair;
    }
    if (!known) { line_flag(&A.head->decline, li, MC_TRAINROWS_DECLINE_PAIR); return -1; }
    int lb = t5 + 1, le = t6;                                     // columns[6].strip(): blanks are the only whitespace a line still holds
    while (lb < le && t[b + lb] == ' ') ++lb;
    while (le > lb && t[b + le - 1] == ' ') --le;
    KeyHash H;                                                    // the label's bytes
    H.span(t + b + lb, le - lb);
    const int nf = commas + 1;
    const bool kept = nf >= 6 && !has0;
    if (kept && nf > MC_TRAINROWS_MAX_FEATURES) { line_flag(&A.head->decline, li, MC_TRAINROWS_DECLINE_FEATURES); return -1; }
    A.row[li] = make_uint4((uint32_t)(t3 + 1) | ((uint32_t)t4 << 16), (uint32_t)cb | ((uint32_t)cn << 16), (uint32_t)lb | ((uint32_t)(le - lb) << 16),
                           (uint32_t)(nf > 65535 ? 65535 : nf) | ((kept ? TR_F_KEPT : 0u) << 16));
    A.hash[li] = H.done(A.hash_mask);
    if (kept) {
        const unsigned long long mine = ((unsigned long long)li << 8) | (unsigned long long)nf;
        if (mine < A.head->first_kept) atomicMin(&A.head->first_kept, mine);      // (the value only falls: a stale one costs an atomic, no more)
    }
    return kept ? cn : -1;
}

__global__ __launch_bounds__(256) void kt_parse(TrArgs A) {
    int cn = -1;
    const bool in_place = staged_lines<TR_STAGE>(A.text, A.n_bytes, A.line_start, A.n_lines, A.n_nl,
                                                 [&](const char *t, int64_t adj, int64_t li) { cn = tr_parse_line(A, t, adj, li); });
    if (in_place && threadIdx.x == 0) atomicAdd(&A.head->in_place, 1u);
    for (int o = 32; o > 0; o >>= 1) cn = max(cn, __shfl_xor(cn, o));
    if ((threadIdx.x & 63) == 0 && cn > 0) atomicMax(&A.head->max_ctx, cn);
}

__device__ __forceinline__ bool tr_same_label(const TrArgs &A, int64_t a, int64_t b) {
    const uint32_t za = A.row[a].z, zb = A.row[b].z;
    if ((za >> 16) != (zb >> 16)) return false;
    return same_bytes(A.text + A.line_start[a] + (za & 0xffffu), A.text + A.line_start[b] + (zb & 0xffffu), (int)(za >> 16));
}

__global__ __launch_bounds__(256) void kt_intern(TrArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines) return;
    TrHead *H = A.head;
    const uint64_t h = A.hash[li];
    const KtHit hit = kt_claim(H->table, TR_SLOTS - 1, h, li, [&](int64_t r) { return A.hash[r] == h && tr_same_label(A, li, r); });
    if (hit.slot < 0) {                                       // every slot holds another label: far more labels than a file may have
        atomicAdd(&H->n_claimed, 1000u);
        A.slot[li] = 0;
        return;
    }
    if (hit.claimed) atomicAdd(&H->n_claimed, 1u);
    A.slot[li] = (uint8_t)hit.slot;
    if ((unsigned long long)li < H->first[hit.slot]) atomicMin(&H->first[hit.slot], (unsigned long long)li);
}

// is line li kept, and which label does it carry (bounds, flags, the host's order of the slots)
__device__ __forceinline__ bool tr_kept(const TrArgs &A, int64_t li, int *id, uint4 *row) {
    *id = -1;
    if (li >= A.n_lines) return false;
    *row = A.row[li];
    *id = (int)A.head->id_of_slot[A.slot[li]];
    return ((row->w >> 16) & TR_F_KEPT) != 0;
}

__global__ __launch_bounds__(256) void kt_count(TrArgs A) {
    __shared__ unsigned s_cnt[MC_TRAINROWS_MAX_LABELS];
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < MC_TRAINROWS_MAX_LABELS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int id;
    uint4 row;
    const bool kept = tr_kept(A, li, &id, &row);
    if (kept && (int)(row.w & 0xffffu) != A.nf) line_flag(&A.head->decline, li, MC_TRAINROWS_DECLINE_FEATURES);
    for (int L = 0; L < A.n_labels; ++L) {
        const unsigned long long bal = __ballot(kept && id == L);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&s_cnt[L], (unsigned)__popcll(bal));
    }
    __syncthreads();
    if ((int)threadIdx.x < A.n_labels) A.blk_cnt[(int64_t)threadIdx.x * A.nblk + blockIdx.x] = (long long)s_cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void kt_rank(TrArgs A) {
    __shared__ unsigned s_w[4][MC_TRAINROWS_MAX_LABELS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int id;
    uint4 row;
    const bool kept = tr_kept(A, li, &id, &row);
    unsigned before_me = 0;
    for (int L = 0; L < A.n_labels; ++L) {
        const unsigned long long bal = __ballot(kept && id == L);
        if (lane == 0) s_w[wave][L] = (unsigned)__popcll(bal);
        if (id == L) before_me = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (!kept) return;
    long long at = A.blk_off[(int64_t)id * A.nblk + blockIdx.x] + before_me;
    for (int w = 0; w < wave; ++w) at += s_w[w][id];
    if (at >= A.n_kept) return;                                // (cannot be: the scan counted the same rows)
    A.row_line[at] = (uint32_t)li;
    // the feature tokens: (begin, end) of the field are offsets from the line's start
    const char *t = A.text + A.line_start[li];
    const int fb = (int)(row.x & 0xffffu), fe = (int)(row.x >> 16);
    uint32_t *tok = A.tok + at * A.nf;
    int j = 0, start = fb;
    for (int i = fb; i <= fe; ++i)
        if (i == fe || t[i] == ',') {
            if (j < A.nf) tok[j] = (uint32_t)start | ((uint32_t)(i - start) << 16);
            ++j;
            start = i + 1;
        }
}

// a lane per number of the result; the lane of a row's first number also copies the row's context
__global__ __launch_bounds__(256) void kt_place(TrArgs A) {
    const int64_t base = (int64_t)blockIdx.x * 256;
    const int64_t row0 = base / A.nf;                           // (uniform: one 64-bit division a workgroup)
    const unsigned local = (unsigned)(base - row0 * A.nf) + threadIdx.x;
    const int64_t xrow = row0 + local / (unsigned)A.nf;
    const int j = (int)(local % (unsigned)A.nf);
    if (xrow >= A.n_kept) return;
    const int64_t li = A.row_line[xrow];
    const char *t = A.text + A.line_start[li];
    const uint32_t tk = A.tok[xrow * A.nf + j];
    double v = 0.0;
    if (!dc_parse(t + (tk & 0xffffu), (int)(tk >> 16), &v)) line_flag(&A.head->decline, li, MC_TRAINROWS_DECLINE_NUMBER);
    A.X[xrow * A.nf + j] = v;
    if (j == 0) {
        const uint32_t y = A.row[li].y;
        const char *c = t + (y & 0xffffu);
        const int cn = (int)(y >> 16);
        char *dst = A.ctx + xrow * A.ctx_w;
        for (int i = 0; i < A.ctx_w; ++i) dst[i] = i < cn ? c[i] : (char)0;
    }
}

// mc_decimal.h alone: a lane per token
__global__ __launch_bounds__(256) void k_dc_probe(const char *__restrict__ text, int64_t n_bytes, const long long *__restrict__ off,
                                                  const int32_t *__restrict__ len, int64_t n, double *__restrict__ out, uint8_t *__restrict__ ok) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long o = off[i];
    const int32_t l = len[i];
    double v = 0.0;
    int good = 0;
    if (o >= 0 && l >= 0 && o <= n_bytes && (long long)l <= n_bytes - o) good = dc_parse(text + o, l, &v);
    out[i] = good ? v : 0.0;
    ok[i] = (uint8_t)good;
}

const char *tr_reason_text(int reason) {
    switch (reason) {
    case MC_TRAINROWS_DECLINE_HIGH_BYTE: return "a byte >= 0x80";
    case MC_TRAINROWS_DECLINE_CONTROL: return "a control byte other than tab and newline";
    case MC_TRAINROWS_DECLINE_FIELDS: return "a line with fewer than 7 tab-separated fields";
    case MC_TRAINROWS_DECLINE_PAIR: return "a context whose centre pair is not an accepted one";
    case MC_TRAINROWS_DECLINE_NUMBER: return "a kept row with a number outside the exact decimal reader's forms";
    case MC_TRAINROWS_DECLINE_FEATURES: return "kept rows with differing feature counts, or more than 64 features";
    case MC_TRAINROWS_DECLINE_CONTEXT: return "a context longer than 63 bytes";
    case MC_TRAINROWS_DECLINE_LABELS: return "more than 16 distinct labels";
    case MC_TRAINROWS_DECLINE_LONG_LINE: return "a line longer than 65535 bytes";
    case MC_TRAINROWS_DECLINE_ROWS: return "more lines than rows are numbered for (2^31 - 2)";
    case MC_TRAINROWS_DECLINE_MEMORY: return "the text and its outputs do not fit into free device memory";
    }
    return "unknown";
}

int tr_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    return decline(c->tr.stats, status, "reader", tr_reason_text(reason), reason, line);
}

int tr_decline_head(mc_ctx *c, int32_t *status, const TrHead &h) {
    return tr_decline(c, status, decline_reason(h.decline), decline_line(h.decline));
}

// The text is on the device (d_text[0, n), padded; copies enqueued on c->up_stream): everything behind that
int tr_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const char *pairs, int32_t n_pairs, mc_train_rows_view *V, int32_t *status) {
    mc_train_rows_stats &S = c->tr.stats;
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    const auto t_kernels = std::chrono::steady_clock::now();
    if (n == 0) return 0;                                     // no line, no label: an empty file
    TrHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline = h.first_kept = ~0ull;
    for (int s = 0; s < TR_SLOTS; ++s) h.first[s] = ~0ull;
    for (int k = 0; k < n_pairs; ++k) h.pairs[k] = (uint16_t)((unsigned char)pairs[2 * k] | ((unsigned)(unsigned char)pairs[2 * k + 1] << 8));
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, d_text, n, &d_head->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t n_nl = h.kp.n_newlines;
    if (too_many_lines(n_nl)) return tr_decline(c, status, MC_TRAINROWS_DECLINE_ROWS, -1);
    // per line: the start, the row, the hash, the slot; per workgroup the counts and their offsets
    if (!device_fits((size_t)(n_nl + 2) * (8 + 16 + 8 + 1 + 1) + ((size_t)1 << 20))) return tr_decline(c, status, MC_TRAINROWS_DECLINE_MEMORY, -1);
    TrArgs A = {};
    if (int rc = lines_starts(pool, st, d_text, n, n_nl, tile_off, &d_head->kp, &line_start)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t n_lines = h.kp.n_lines;
    S.n_lines = n_lines;
    A.text = d_text; A.n_bytes = n; A.n_lines = n_lines; A.n_nl = n_nl; A.line_start = line_start; A.head = d_head;
    A.n_pairs = n_pairs;
    A.hash_mask = ~0ull;
    if (const char *e = getenv("MCALLER_TRAINROWS_HASH_MASK")) A.hash_mask = strtoull(e, nullptr, 16);
    const size_t nl = (size_t)n_lines;
    const unsigned lb = (unsigned)((n_lines + 255) / 256);
    A.nblk = lb;
    if (pool.get(&A.row, nl) || pool.get(&A.hash, nl) || pool.get(&A.slot, nl)) return -10;
    hipLaunchKernelGGL(kt_parse, dim3(lb), dim3(256), TR_STAGE + 16, st, A);
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.in_place_blocks = (int32_t)h.in_place;
    if (h.decline != ~0ull) return tr_decline_head(c, status, h);
    hipLaunchKernelGGL(kt_intern, dim3(lb), dim3(256), 0, st, A);
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.n_claimed > MC_TRAINROWS_MAX_LABELS) return tr_decline(c, status, MC_TRAINROWS_DECLINE_LABELS, -1);
    // the labels in the order of the lines that registered them
    int slots[MC_TRAINROWS_MAX_LABELS], n_labels = 0;
    for (int s = 0; s < TR_SLOTS; ++s)
        if (h.table[s] != 0ull) slots[n_labels++] = s;
    std::sort(slots, slots + n_labels, [&](int a, int b) { return h.first[a] < h.first[b]; });
    for (int i = 0; i < n_labels; ++i) h.id_of_slot[slots[i]] = (uint8_t)i;
    HIP_TRY(hipMemcpyAsync(d_head->id_of_slot, h.id_of_slot, sizeof h.id_of_slot, hipMemcpyHostToDevice, st));
    S.n_labels = n_labels;
    A.n_labels = n_labels;
    A.nf = h.first_kept != ~0ull ? (int)(h.first_kept & 0xff) : 0;
    S.n_features = A.nf;
    A.ctx_w = std::max(1, h.max_ctx);
    const size_t n_cnt = (size_t)n_labels * lb;
    if (pool.get(&A.blk_cnt, n_cnt) || pool.get(&A.blk_off, n_cnt)) return -10;
    hipLaunchKernelGGL(kt_count, dim3(lb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.blk_cnt, (int64_t)n_cnt, A.blk_off, &d_head->n_kept);
    HIP_TRY(hipMemcpyAsync(&h, d_head, sizeof h, hipMemcpyDeviceToHost, st));
    // a label's rows: the offset of the label behind it less its own -- the first workgroup's offsets, one small copy a label
    long long first_off[MC_TRAINROWS_MAX_LABELS + 1] = {};
    for (int i = 0; i < n_labels; ++i) HIP_TRY(hipMemcpyAsync(&first_off[i], A.blk_off + (size_t)i * lb, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h.decline != ~0ull) return tr_decline_head(c, status, h);
    const int64_t n_kept = h.n_kept;
    first_off[n_labels] = n_kept;
    S.n_kept = n_kept;
    A.n_kept = n_kept;
    if (n_kept > 0) {
        const size_t nk = (size_t)n_kept, nx = nk * (size_t)A.nf;
        if (!device_fits(nk * 4 + nx * 12 + nk * (size_t)A.ctx_w)) return tr_decline(c, status, MC_TRAINROWS_DECLINE_MEMORY, -1);
        if (pool.get(&A.row_line, nk) || pool.get(&A.tok, nx) || pool.get(&A.X, nx) || pool.get(&A.ctx, nk * (size_t)A.ctx_w)) return -10;
        hipLaunchKernelGGL(kt_rank, dim3(lb), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kt_place, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.decline != ~0ull) return tr_decline_head(c, status, h);
    }
    S.ms_kernels = ms_since(t_kernels);
    const auto t_d2h = std::chrono::steady_clock::now();
    // the labels' bytes: where the row that claimed the slot has them
    c->tr.labels.clear();
    V->label_off[0] = 0;
    for (int i = 0; i < n_labels; ++i) {
        const int64_t r = (int64_t)(h.table[slots[i]] & 0xffffffffull) - 1;
        uint4 row;
        long long ls = 0;
        HIP_TRY(hipMemcpy(&row, A.row + r, sizeof row, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&ls, line_start + r, 8, hipMemcpyDeviceToHost));
        const size_t at = c->tr.labels.size(), ln = row.z >> 16;
        c->tr.labels.resize(at + ln);
        if (ln) HIP_TRY(hipMemcpy(&c->tr.labels[at], d_text + ls + (row.z & 0xffffu), ln, hipMemcpyDeviceToHost));
        V->label_off[i + 1] = (int32_t)c->tr.labels.size();
        V->n_rows[i] = first_off[i + 1] - first_off[i];
        V->first_line[i] = (int64_t)h.first[slots[i]];
    }
    if (n_kept > 0) {
        const size_t xb = (size_t)n_kept * (size_t)A.nf * 8, cb = (size_t)n_kept * (size_t)A.ctx_w;
        if (int rc = c->tr.X.need(xb)) return rc;
        if (int rc = c->tr.ctx.need(cb)) return rc;
        HIP_TRY(hipMemcpyAsync(c->tr.X.get<double>(), A.X, xb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c->tr.ctx.get<char>(), A.ctx, cb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        V->X = c->tr.X.get<double>();
        V->contexts = c->tr.ctx.get<char>();
    }
    S.ms_d2h = ms_since(t_d2h);
    V->n_labels = n_labels;
    V->n_features = n_kept > 0 ? A.nf : 0;
    V->ctx_width = n_kept > 0 ? A.ctx_w : 0;
    V->n_rows_total = n_kept;
    V->label_bytes = c->tr.labels.data();
    return 0;
}

// what the entry point runs: the text of `src` onto the device and through tr_run
int tr_call(mc_ctx *c, const mc_text_source &src, const char *pairs, int32_t n_pairs, mc_train_rows_view *out, int32_t *status) {
    mc_train_rows_stats &S = c->tr.stats;
    return pipeline_call(c, S, status, "training rows", (size_t)64 << 20, [&] { *out = mc_train_rows_view(); }, [&](Call &K) -> int {
        S.n_bytes = src.n_bytes;
        if (n_pairs < 0 || n_pairs > MC_TRAINROWS_MAX_PAIRS || (n_pairs > 0 && !pairs)) {
            mc_set_error("mc_train_rows: 0 to %d centre pairs", MC_TRAINROWS_MAX_PAIRS);
            return -12;
        }
        if (!device_fits((size_t)src.n_bytes + 4096)) return tr_decline(c, status, MC_TRAINROWS_DECLINE_MEMORY, -1);
        char *d_text = nullptr;
        if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;
        K.feed.times(S, K.t0);
        return tr_run(c, K.pool, d_text, src.n_bytes, pairs, n_pairs, out, status);
    });
}

}  // namespace

extern "C" int mc_train_rows(mc_ctx *c, const mc_text_source *src, const char *pairs, int32_t n_pairs, mc_train_rows_view *out,
                             int32_t *status) {
    if (!c || !out || !status) {
        mc_set_error("mc_train_rows: bad arguments");
        return -12;
    }
    mc_text_source s = {};
    if (int rc = text_source("mc_train_rows", src, &s)) return rc;
    return tr_call(c, s, pairs, n_pairs, out, status);
}

extern "C" int mc_train_rows_last_stats(mc_ctx *c, mc_train_rows_stats *out) {
    return stats_out("mc_train_rows_last_stats", c, out, &mc_ctx::tr, &TrainPipe::stats);
}

extern "C" int mc_train_rows_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::tr); }

extern "C" int mc_parse_doubles_device(mc_ctx *c, const char *text, int64_t n_bytes, const int64_t *off, const int32_t *len, int64_t n,
                                       double *out, uint8_t *ok) {
    if (!c || n < 0 || n_bytes < 0 || (n_bytes > 0 && !text) || (n > 0 && (!off || !len || !out || !ok))) {
        mc_set_error("mc_parse_doubles_device: bad arguments");
        return -12;
    }
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Pool pool("decimal probe");
    char *d_text = nullptr;
    long long *d_off = nullptr;
    int32_t *d_len = nullptr;
    double *d_out = nullptr;
    uint8_t *d_ok = nullptr;
    if (pool.get(&d_text, (size_t)n_bytes + 1) || pool.get(&d_off, (size_t)n) || pool.get(&d_len, (size_t)n) || pool.get(&d_out, (size_t)n) ||
        pool.get(&d_ok, (size_t)n))
        return -10;
    hipStream_t st = c->stream;
    if (n_bytes > 0) HIP_TRY(hipMemcpyAsync(d_text, text, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, off, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dc_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const char *)d_text, n_bytes, (const long long *)d_off,
                       (const int32_t *)d_len, n, d_out, d_ok);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ok, d_ok, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
