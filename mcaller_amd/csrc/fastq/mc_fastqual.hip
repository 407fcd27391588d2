// mc_fastqual.hip -- the read qualities of a FASTQ file, made on the GPU: one (key, mean phred) pair per record, what
// read_qual.py:15-47 builds line by line in Python (C ABI: mc_fastq_quality, mc_fastq_quality_last_stats,
// mc_fastq_quality_release; Python: Device.fastq_qualities, read_qual.extract_read_quality_device).  The unit stands in csrc/fastq/,
// beside the units of the passes like csrc/bed/, csrc/train/ and csrc/merge/: no pass runs its kernels.
//
// The rules of a record, and what makes the reader decline (status 1, mc_last_error; MC_FASTQ_DECLINE_*), are mc_fastqrec.h's --
// the same functions mc_fastq_records_host runs on the CPU.  Beyond them the call declines for 2^31 - 2 lines or more and for a text
// that does not fit into free device memory beside its outputs: the WHOLE text stays resident.
//
// The steps (R = records, P = FQ_PIECE bytes):
//   kp_count / kp_scan / kp_starts   line starts (the device parser's kernels: mc_lines.h, launched by mc_textfeed.h)
//   kfq_class    a stream over the whole text, 64 bytes a lane in four 16-byte loads: the byte classes and the '\r' rule four bytes
//                at a time (the byte behind a word and behind the tile is looked at too), the last byte that is no blank, tab or
//                line break by atomicMax.  Only a lane that found something walks its bytes: line_flag (mc_textdev.h)
//   kfq_last     one lane: the line of that last byte -> R
//   kfq_records  a lane per record: fq_record on its four line spans (the title line, the two ends of the sequence line, one byte
//                of the third) -> the key's span and length + 1 (kfq_keylen is merged into it: the title is read once), the
//                quality line's span, its pieces ceil(n / P), a zeroed 64-bit sum
//   kp_scan x 2  the pieces and the key lengths, exclusive
//   kfq_piecemap a lane per record: the record of each of its pieces (a read of 10^6 bases has 245)
//   kfq_sum      a WAVE per piece: 16-byte loads from the aligned address at or below the piece's first byte, the bytes outside the
//                piece masked off, byte sums by v_sad_u8, one 64-bit integer atomicAdd a piece into its record's sum -- integer
//                addition: the result does not depend on the order of arrival.  Only quality lines are read
//   kfq_finish   a lane per record: fq_mean
//   kfq_keys     a lane per record: its key and a '\n' into the pool; the offsets' last entry
// wave64; no library sort or scan; every buffer, event and stream through the owners of mc_own.h.
// The host side around the kernels -- a file's way onto the device through the context's two pinned stages, the line starts, the
// head's way back, the decline, the clock -- is mc_textfeed.h's, shared with the other units that take a whole text file.
#include "../mc_textfeed.h"
#include "../mc_fastqrec.h"

#include <cstring>

namespace {

struct FqHead {                              // device-side result block (copied to the host as it is)
    KpHead kp;                               // n_newlines (kp_scan), n_lines (kp_starts)
    unsigned long long decline;              // min over the offending lines of line << 8 | reason (~0: none)
    unsigned long long last_off1;            // 1 + the offset of the last byte that is no blank, tab or line break (0: none)
    long long last_line;                     // its line (-1: none)
    long long n_pieces, pool_bytes;          // totals of the two scans
};

struct FqArgs {
    const char *text;
    int64_t n_bytes, n_lines, n_nl, R;
    const long long *line_start;
    FqHead *head;
    // per record
    long long *key_b, *key_len1, *qual_b, *qual_n, *pieces, *piece_off, *key_off;
    unsigned long long *sum;
    double *mean;
    // per piece; the keys
    uint32_t *piece_rec;
    int64_t n_pieces;
    char *pool;
};

// the bytes [b, e) one by one: the declines with their lines, the last byte that fills a line -> 1 + its offset, 0: none
__device__ __noinline__ unsigned long long fq_class_bytes(const char *__restrict__ text, int64_t n, const long long *__restrict__ line_start,
                                                          int64_t n_nl, FqHead *head, int64_t b, int64_t e) {
    unsigned long long last1 = 0;
    int64_t line = -1;
    for (int64_t i = b; i < e; ++i) {
        const unsigned c = (unsigned char)text[i];
        const int reason = fq_byte_reason(c, i + 1 < n ? (int)(unsigned char)text[i + 1] : -1);
        if (reason) {
            if (line < 0) line = fq_line_of(line_start, n_nl, i);
            line_flag(&head->decline, line, reason);
        }
        if (!fq_blank(c) && c != '\r' && c != '\n') last1 = (unsigned long long)i + 1;
        if (c == '\n' && line >= 0) ++line;
    }
    return last1;
}

__global__ __launch_bounds__(KP_THREADS) void kfq_class(const char *__restrict__ text, int64_t n, const long long *__restrict__ line_start,
                                                        int64_t n_nl, FqHead *__restrict__ head) {
    __shared__ unsigned long long s_last[KP_THREADS / 64];
    const int64_t b = (int64_t)blockIdx.x * KP_TILE + threadIdx.x * 64;
    unsigned long long last1 = 0;
    if (b + 64 <= n) {
        uint32_t w[16];
        const uint4 *p = reinterpret_cast<const uint4 *>(text + b);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = p[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
        const unsigned behind = b + 64 < n ? (unsigned)(unsigned char)text[b + 64] : 0u;      // the byte behind the lane's: across the word, the lane, the tile
        uint32_t any = 0, top_bits = 0;
        int top = -1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t cr, nl, fill;
            const uint32_t bad = fq_bad_bits(w[i], &cr, &nl, &fill);
            const unsigned next = i < 15 ? (w[i < 15 ? i + 1 : 15] & 0xffu) : behind;
            uint32_t lone = (cr << 8) & ~nl;                   // a '\r' in bytes 0..2: the byte above it is no '\n'
            if ((cr >> 31) && next != '\n') lone |= 1u;
            any |= bad | lone;
            const uint32_t fills = ~fill & 0x80808080u;
            if (fills) { top = i; top_bits = fills; }
        }
        if (top >= 0) last1 = (unsigned long long)(b + 4 * top + ((31 - __clz(top_bits)) >> 3)) + 1;
        if (any) (void)fq_class_bytes(text, n, line_start, n_nl, head, b, b + 64);
    } else if (b < n) {
        last1 = fq_class_bytes(text, n, line_start, n_nl, head, b, n);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(last1, o);
        last1 = v > last1 ? v : last1;
    }
    if ((threadIdx.x & 63) == 0) s_last[threadIdx.x >> 6] = last1;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = s_last[0];
        for (int i = 1; i < KP_THREADS / 64; ++i) m = s_last[i] > m ? s_last[i] : m;
        if (m) atomicMax(&head->last_off1, m);
    }
}

__global__ void kfq_last(const long long *__restrict__ line_start, int64_t n_nl, FqHead *__restrict__ head) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        head->last_line = head->last_off1 ? (long long)fq_line_of(line_start, n_nl, (int64_t)head->last_off1 - 1) : -1;
}

__global__ __launch_bounds__(256) void kfq_records(FqArgs A) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.R) return;
    int64_t b[4], e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fq_line_span(A.text, A.n_bytes, A.line_start, A.n_nl, A.n_lines, 4 * r + i, &b[i], &e[i]);
    FqRecord rec;
    const unsigned long long code = fq_record(A.text, r, b, e, &rec);
    if (code) {
        line_flag(&A.head->decline, (long long)(code >> 8), (int)(code & 0xff));       // (fq_record's code: fq_code of the line and the reason)
        rec.key_n = 0; rec.qual_n = 0;                         // (nothing behind this kernel runs on a declined text; the arrays are whole all the same)
    }
    A.key_b[r] = rec.key_b;
    A.key_len1[r] = rec.key_n + 1;
    A.qual_b[r] = rec.qual_b;
    A.qual_n[r] = rec.qual_n;
    A.pieces[r] = (rec.qual_n + FQ_PIECE - 1) / FQ_PIECE;
    A.sum[r] = 0ull;
}

__global__ __launch_bounds__(256) void kfq_piecemap(FqArgs A) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.R) return;
    const long long at = A.piece_off[r], k = A.pieces[r];
    for (long long j = 0; j < k; ++j)
        if (at + j < A.n_pieces) A.piece_rec[at + j] = (uint32_t)r;
}

__device__ __forceinline__ uint32_t fq_sum4(uint32_t w, uint32_t acc) {       // acc + the four bytes of w
    return __builtin_amdgcn_sad_u8(w, 0u, acc);
}

// the bytes of the word at address `at` that lie in [s, e): the others zeroed
__device__ __forceinline__ uint32_t fq_inside(uint32_t w, int64_t at, int64_t s, int64_t e) {
    const int lo = (int)max((int64_t)0, min((int64_t)4, s - at)), hi = (int)max((int64_t)0, min((int64_t)4, e - at));
    if (hi <= lo) return 0u;
    const uint32_t below_hi = hi == 4 ? 0xffffffffu : (1u << (8 * hi)) - 1u;
    const uint32_t below_lo = (1u << (8 * lo)) - 1u;           // (lo < hi <= 4: lo <= 3)
    return w & below_hi & ~below_lo;
}

__global__ __launch_bounds__(256) void kfq_sum(FqArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // (the same for the whole wave)
    if (p >= A.n_pieces) return;
    const uint32_t r = A.piece_rec[p];
    if ((int64_t)r >= A.R) return;
    const int64_t j = p - A.piece_off[r];
    const int64_t qb = A.qual_b[r], qn = A.qual_n[r];
    const int64_t s = qb + j * FQ_PIECE;
    const int64_t e = min(s + (int64_t)FQ_PIECE, qb + qn);
    if (j < 0 || s >= e || e > A.n_bytes) return;              // (cannot be: the scan counted these pieces)
    uint32_t acc = 0;
    // whole 16-byte groups from the aligned address at or below s: the text's buffer begins aligned and is padded behind its end
    for (int64_t a = (s & ~(int64_t)15) + (int64_t)lane * 16; a < e; a += 64 * 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(A.text + a);
        if (a >= s && a + 16 <= e) {
            acc = fq_sum4(v.x, acc); acc = fq_sum4(v.y, acc); acc = fq_sum4(v.z, acc); acc = fq_sum4(v.w, acc);
        } else {                                               // the piece's unaligned head or tail
            acc = fq_sum4(fq_inside(v.x, a, s, e), acc); acc = fq_sum4(fq_inside(v.y, a + 4, s, e), acc);
            acc = fq_sum4(fq_inside(v.z, a + 8, s, e), acc); acc = fq_sum4(fq_inside(v.w, a + 12, s, e), acc);
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);       // (a piece's bytes sum to less than 2^21)
    if (lane == 0) atomicAdd(&A.sum[r], (unsigned long long)acc);
}

__global__ __launch_bounds__(256) void kfq_finish(FqArgs A) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.R) return;
    A.mean[r] = fq_mean((uint64_t)A.sum[r], (int64_t)A.qual_n[r]);
}

__global__ __launch_bounds__(256) void kfq_keys(FqArgs A) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) A.key_off[A.R] = A.head->pool_bytes;
    if (r >= A.R) return;
    const long long at = A.key_off[r], k = A.key_len1[r] - 1;
    if (at < 0 || at + k + 1 > A.head->pool_bytes) return;     // (cannot be: the scan counted these bytes)
    const char *src = A.text + A.key_b[r];
    for (long long i = 0; i < k; ++i) A.pool[at + i] = src[i];
    A.pool[at + k] = '\n';
}

int fq_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    return decline(c->fq.stats, status, "reader", fq_reason_text(reason), reason, line);
}

int fq_decline_head(mc_ctx *c, int32_t *status, const FqHead &h) {
    return fq_decline(c, status, decline_reason(h.decline), decline_line(h.decline));
}

// The text is on the device (d_text[0, n), its buffer aligned and padded; copies enqueued on c->up_stream): everything behind that
int fq_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, mc_fastq_quality_view *V, int32_t *status) {
    mc_fastq_quality_stats &S = c->fq.stats;
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    const auto t_kernels = std::chrono::steady_clock::now();
    if (n == 0) return 0;                                     // no line, no record: an empty file
    FqHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline = FQ_NO_DECLINE;
    h.last_line = -1;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    const int64_t n_tiles = (n + KP_TILE - 1) / KP_TILE;
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, d_text, n, &d_head->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t n_nl = h.kp.n_newlines;
    if (too_many_lines(n_nl)) return fq_decline(c, status, MC_FASTQ_DECLINE_ROWS, -1);
    if (!device_fits((size_t)(n_nl + 2) * 8 + ((size_t)1 << 20))) return fq_decline(c, status, MC_FASTQ_DECLINE_MEMORY, -1);
    if (int rc = lines_starts(pool, st, d_text, n, n_nl, tile_off, &d_head->kp, &line_start)) return rc;
    hipLaunchKernelGGL(kfq_class, dim3((unsigned)n_tiles), dim3(KP_THREADS), 0, st, d_text, n, (const long long *)line_start, n_nl, d_head);
    hipLaunchKernelGGL(kfq_last, dim3(1), dim3(64), 0, st, (const long long *)line_start, n_nl, d_head);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_lines = h.kp.n_lines;
    const int64_t R = h.last_line < 0 ? 0 : h.last_line / 4 + 1;
    if (R == 0) {                                             // nothing but blanks, tabs and line breaks -- or bytes that decline
        if (h.decline != FQ_NO_DECLINE) return fq_decline_head(c, status, h);
        S.ms_kernels = ms_since(t_kernels);
        return 0;
    }
    FqArgs A = {};
    A.text = d_text; A.n_bytes = n; A.n_lines = h.kp.n_lines; A.n_nl = n_nl; A.R = R; A.line_start = line_start; A.head = d_head;
    const size_t nr = (size_t)R;
    if (!device_fits(nr * 80 + ((size_t)1 << 20))) return fq_decline(c, status, MC_FASTQ_DECLINE_MEMORY, -1);
    if (pool.get(&A.key_b, nr) || pool.get(&A.key_len1, nr) || pool.get(&A.qual_b, nr) || pool.get(&A.qual_n, nr) || pool.get(&A.pieces, nr) ||
        pool.get(&A.piece_off, nr) || pool.get(&A.key_off, nr + 1) || pool.get(&A.sum, nr) || pool.get(&A.mean, nr))
        return -10;
    const unsigned rb = (unsigned)((R + 255) / 256);
    hipLaunchKernelGGL(kfq_records, dim3(rb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.pieces, R, A.piece_off, &d_head->n_pieces);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.key_len1, R, A.key_off, &d_head->pool_bytes);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.decline != FQ_NO_DECLINE) return fq_decline_head(c, status, h);
    A.n_pieces = h.n_pieces;
    S.n_records = R;
    S.n_pieces = h.n_pieces;
    const size_t np = (size_t)h.n_pieces, pb = (size_t)h.pool_bytes;
    if (!device_fits(np * 4 + pb + ((size_t)1 << 20))) return fq_decline(c, status, MC_FASTQ_DECLINE_MEMORY, -1);
    if (pool.get(&A.piece_rec, np) || pool.get(&A.pool, pb)) return -10;
    if (np > 0) {
        hipLaunchKernelGGL(kfq_piecemap, dim3(rb), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kfq_sum, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, st, A);
    }
    hipLaunchKernelGGL(kfq_finish, dim3(rb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kfq_keys, dim3(rb), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    S.ms_kernels = ms_since(t_kernels);
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = c->fq.pool.need(pb)) return rc;
    if (int rc = c->fq.off.need((nr + 1) * 8)) return rc;
    if (int rc = c->fq.mean.need(nr * 8)) return rc;
    HIP_TRY(hipMemcpyAsync(c->fq.pool.get<char>(), A.pool, pb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->fq.off.get<int64_t>(), A.key_off, (nr + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->fq.mean.get<double>(), A.mean, nr * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    S.ms_d2h = ms_since(t_d2h);
    V->key_pool = c->fq.pool.get<char>();
    V->key_off = c->fq.off.get<int64_t>();
    V->mean = c->fq.mean.get<double>();
    V->n_records = R;
    return 0;
}

// what the entry point runs: the text of `src` onto the device and through fq_run
int fq_call(mc_ctx *c, const mc_text_source &src, mc_fastq_quality_view *out, int32_t *status) {
    mc_fastq_quality_stats &S = c->fq.stats;
    return pipeline_call(c, S, status, "fastq qualities", (size_t)32 << 20, [&] { *out = mc_fastq_quality_view(); }, [&](Call &K) -> int {
        S.n_bytes = src.n_bytes;
        S.piece_bytes = FQ_PIECE;
        if (!device_fits((size_t)src.n_bytes + 4096)) return fq_decline(c, status, MC_FASTQ_DECLINE_MEMORY, -1);
        char *d_text = nullptr;
        if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;
        K.feed.times(S, K.t0);
        return fq_run(c, K.pool, d_text, src.n_bytes, out, status);
    });
}

}  // namespace

extern "C" int mc_fastq_quality(mc_ctx *c, const mc_text_source *src, mc_fastq_quality_view *out, int32_t *status) {
    if (!c || !out || !status) {
        mc_set_error("mc_fastq_quality: bad arguments");
        return -12;
    }
    mc_text_source s = {};
    if (int rc = text_source("mc_fastq_quality", src, &s)) return rc;
    return fq_call(c, s, out, status);
}

extern "C" int mc_fastq_quality_last_stats(mc_ctx *c, mc_fastq_quality_stats *out) {
    return stats_out("mc_fastq_quality_last_stats", c, out, &mc_ctx::fq, &FastqPipe::stats);
}

extern "C" int mc_fastq_quality_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::fq); }
