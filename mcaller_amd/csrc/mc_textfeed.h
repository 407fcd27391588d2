// mc_textfeed.h -- what the seven units that take whole text files through the GPU share on the host side (bed/mc_bedsum.hip,
// train/mc_trainrows.hip, merge/mc_rowmerge.hip, fastq/mc_fastqual.hip, eval/mc_evalcalls.hip, motifs/mc_motifscan.hip and
// compare/mc_bedcompare.hip, whose .inc files hold five pipelines: the comparison, the alignment map, the currents, the clusters, the read phasing).
// Included by those seven units only, hence the unnamed namespace: nothing here is linked across units.
//
// What the author of another pipeline writes.  In mc_ctx.h a record `XPipe x` with the Grown blocks its results are handed out in,
// its stats and a release().  An entry point that refuses its arguments (-12), takes each of its sources (text_source: the checks
// on a mc_text_source, a file sized) and then runs its body inside the call frame:
//
//     return pipeline_call(c, c->x.stats, status, "x", (size_t)64 << 20, [&] { *out = nullptr; *n_out = 0; }, [&](Call &K) -> int {
//         c->x.stats.n_bytes = src.n_bytes;
//         if (!fits("MCALLER_X_DEVICE_BYTES", n + ...)) return decline(c->x.stats, status, "reader", text, reason, -1);
//         char *d_text = nullptr;
//         if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;        // src: a host text or a file; padded and waited for
//         K.feed.times(c->x.stats, K.t0);                                  // ms_read, ms_h2d
//         lines_count(..); the unit's own kernels; fetch_head(..); too_many_lines(..); lines_starts(..); fetch_head(..);
//         if (h.decline != ~0ull) return decline(.., decline_reason(h.decline), decline_line(h.decline));
//         return fetch_out(c, c->x.out, d_out, n, out, n_out);             // the result into the pipeline's pinned block
//     });
//
// The frame (pipeline_call) selects the device, blanks the stats, the status and -- through the first callable -- the results,
// owns the call's Pool and TextFeed (K.pool, K.feed), and on every way out waits for c->stream before the pool goes, blanks the
// results again unless the call produced some (rc == 0 and *status == 0) and writes ms_total.  Two more entry points are one line
// each: mc_x_last_stats (stats_out) and mc_x_release (release_pipeline).
//
// Several texts behind one another in one buffer: K.feed.put_pair for two whose lines are numbered through (the comparisons, the
// motif finder), or K.feed.send(src, d_dst, &last_byte) for each and then K.feed.pad_and_wait(d_end) (the merge).  The feed's two
// pinned stages and their events are the context's (mc_ctx::text_stages): the calls of the seven units are synchronous and never
// run side by side, so one pair serves them all.
// The device side they share -- the decline word, byte classes, key hash, key table, tab spans, LDS staging -- is mc_textdev.h,
// which comes in through this header; table_slots / table_get below are its key table's host half.
#pragma once
#include "mc_lines.h"
#include "mc_textdev.h"

#include <sys/stat.h>

#include <chrono>

extern "C" int mc_read_file_range(const char *path, int64_t lo, int64_t hi, char *dst, int32_t n_threads);

namespace {

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// does `bytes` more fit into device memory, with a margin for what the runtime and the other buffers of the context take
inline bool device_fits(size_t bytes) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    const size_t margin = (size_t)256 << 20;
    return free_b > margin && bytes <= free_b - margin;
}

// the same behind a test's knob: where the environment variable `knob` holds a positive number, that stands for the free device
// memory (anything else: as if unset)
inline bool fits(const char *knob, size_t bytes) {
    const char *e = getenv(knob);
    const long long have = e ? atoll(e) : 0;
    return have > 0 ? bytes <= (size_t)have : device_fits(bytes);
}

inline int regular_file_size(const char *what, const char *path, int64_t *n) {
    struct stat sb;
    if (!path || stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        mc_set_error("%s: %s is not a readable file", what, path ? path : "(null)");
        return -1;
    }
    *n = (int64_t)sb.st_size;
    return 0;
}

// the device-side result block of a unit onto the host, waited for
template <typename H>
int fetch_head(hipStream_t st, const H *d_head, H &h) {
    HIP_TRY(hipMemcpyAsync(&h, d_head, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// A call declines (status 1, mc_last_error; the host code does the file): the reason and the line (-1: none) into the unit's stats.
// A head's `decline` word is the minimum over the offending lines of line << 8 | reason
template <typename S>
int decline(S &stats, int32_t *status, const char *noun, const char *text, int reason, long long line) {
    stats.decline_reason = reason;
    stats.decline_line = line;
    if (line >= 0) mc_set_error("the device %s declines: %s (line %lld)", noun, text, line + 1);
    else mc_set_error("the device %s declines: %s", noun, text);
    *status = 1;
    return 0;
}
// ... of one of a call's files: decline_file, and the file's noun behind the reason -- nouns[file - 1]; file 0: no file, no noun
template <typename S>
int decline_in_file(S &stats, int32_t *status, const char *noun, const char *text, const char *const *nouns, int reason, int file, long long line) {
    stats.decline_file = file;
    char what[200];
    if (file) snprintf(what, sizeof what, "%s (%s)", text, nouns[file - 1]);
    else snprintf(what, sizeof what, "%s", text);
    return decline(stats, status, noun, what, reason, line);
}
inline int decline_reason(unsigned long long word) { return (int)(word & 0xff); }
inline long long decline_line(unsigned long long word) { return (long long)(word >> 8); }

// ---- a key table (mc_textdev.h): its slots, a power of two of at least `floor` and 2 x keys -- or of at least the number in the
// environment variable `knob`, where that is 1 or more (tests: a table that is too small) -- and the table itself from the pool,
// every slot empty (on the stream) ----
inline uint64_t table_slots(int64_t keys, int64_t floor, const char *knob = nullptr) {
    const char *e = knob ? getenv(knob) : nullptr;
    long long want = e ? atoll(e) : 0;
    if (want < 1) want = std::max<long long>(floor, 2 * keys);
    uint64_t slots = 1;
    while ((long long)slots < want) slots <<= 1;
    return slots;
}
inline int table_get(Pool &pool, hipStream_t st, unsigned long long **table, uint64_t slots) {
    if (pool.get(table, (size_t)slots)) return -10;
    HIP_TRY(hipMemsetAsync(*table, 0, (size_t)slots * 8, st));
    return 0;
}

// ---- the line starts of a text on the device (padded, n > 0), in two halves: a unit puts kernels of its own between them and
// fetches its head once for both.  tile_off: the scan of the first half, which the second reads ----
inline int lines_count(Pool &pool, hipStream_t st, const char *d_text, int64_t n, KpHead *d_kp, long long **tile_off) {
    const int64_t n_tiles = (n + KP_TILE - 1) / KP_TILE;
    long long *tile_cnt = nullptr;
    if (pool.get(&tile_cnt, (size_t)n_tiles) || pool.get(tile_off, (size_t)n_tiles)) return -10;
    hipLaunchKernelGGL(kp_count, dim3((unsigned)n_tiles), dim3(KP_THREADS), 0, st, d_text, n, tile_cnt);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)tile_cnt, n_tiles, *tile_off, &d_kp->n_newlines);
    return 0;
}

inline bool too_many_lines(int64_t n_nl) { return n_nl + 1 >= ((int64_t)1 << 31) - 2; }      // lines are numbered in 32 bits

// line_start[0 .. n_lines] (n_nl + 2 entries of room), KpHead.n_lines: the last line may lack its newline
inline int lines_starts(Pool &pool, hipStream_t st, const char *d_text, int64_t n, int64_t n_nl, const long long *tile_off, KpHead *d_kp,
                        long long **line_start) {
    const int64_t n_tiles = (n + KP_TILE - 1) / KP_TILE, cap_lines = n_nl + 2;
    if (pool.get(line_start, (size_t)cap_lines)) return -10;
    hipLaunchKernelGGL(kp_starts, dim3((unsigned)n_tiles), dim3(KP_THREADS), 0, st, d_text, n, tile_off, *line_start, cap_lines, d_kp);
    return 0;
}

// A source (mcaller_hip.h) as an entry point `what` was given it -> 0 and *out: the source with n_bytes filled in (a file is
// sized); -12: none, a text and a path, a negative size, bytes without a text; -1: a path that is no readable regular file
inline int text_source(const char *what, const mc_text_source *s, mc_text_source *out) {
    if (!s || (s->text && s->path) || (!s->path && (s->n_bytes < 0 || (s->n_bytes > 0 && !s->text)))) {
        mc_set_error("%s: bad arguments", what);
        return -12;
    }
    *out = *s;
    return s->path ? regular_file_size(what, s->path, &out->n_bytes) : 0;
}

// Host texts and files, one behind the other, into device buffers: copies on c->up_stream.  A file goes in blocks through the
// context's two pinned stages in turn: block i is read while block i - 1 is on its way.  A stage is not written again until the
// event recorded behind the copy out of it has completed; the block count runs across the files of a call.
struct TextFeed {
    mc_ctx *c;
    size_t max_block;                            // a file's step: the caller's, or MCALLER_TEXT_STAGE_BYTES (tests; Pinned's 256 or more)
    double ms_read = 0;                          // in mc_read_file_range
    int64_t n_blocks = 0;                        // blocks sent: block i goes through stage i & 1
    TextFeed(mc_ctx *ctx, size_t caller_max) : c(ctx), max_block(caller_max) {
        const char *e = getenv("MCALLER_TEXT_STAGE_BYTES");
        const long long want = e ? atoll(e) : 0;                    // (empty, no number or below 256: as if unset)
        if (want >= 256) max_block = (size_t)want;
    }
    size_t block_for(int64_t n) const { return std::min<size_t>((size_t)std::max<int64_t>(n, 4096), max_block); }
    int stages(size_t block) {                   // the two stages hold a block each; their events exist
        TextStages &T = c->text_stages;
        if (T.cap < block) {
            T.cap = 0;
            for (Pinned &p : T.stage)
                if (int rc = p.alloc(block)) return rc;
            T.cap = block;
        }
        for (Event &e : T.ev)
            if (!e.e)
                if (int rc = e.create()) return rc;
        return 0;
    }
    int text(const char *src, int64_t n, char *d_dst) {
        if (n > 0) HIP_TRY(hipMemcpyAsync(d_dst, src, (size_t)n, hipMemcpyHostToDevice, c->up_stream));
        return 0;
    }
    // last_byte: the file's last byte as it was read (n > 0)
    int file(const char *path, int64_t n, char *d_dst, char *last_byte = nullptr) {
        const int64_t step = (int64_t)block_for(n);
        if (int rc = stages((size_t)step)) return rc;
        TextStages &T = c->text_stages;
        for (int64_t lo = 0; lo < n; lo += step, ++n_blocks) {
            const int turn = (int)(n_blocks & 1);
            const int64_t hi = std::min<int64_t>(n, lo + step);
            if (n_blocks >= 2) HIP_TRY(hipEventSynchronize(T.ev[turn]));      // the copy out of this stage is done
            const auto tr = std::chrono::steady_clock::now();
            const int rc = mc_read_file_range(path, lo, hi, T.stage[turn].get<char>(), 0);
            ms_read += ms_since(tr);
            if (rc) {
                (void)hipStreamSynchronize(c->up_stream);                     // (nothing is on its way when the caller's pool goes)
                return rc;
            }
            if (last_byte && hi == n) *last_byte = T.stage[turn].get<char>()[hi - lo - 1];
            HIP_TRY(hipMemcpyAsync(d_dst + lo, T.stage[turn].p, (size_t)(hi - lo), hipMemcpyHostToDevice, c->up_stream));
            HIP_TRY(hipEventRecord(T.ev[turn], c->up_stream));
        }
        return 0;
    }
    int send(const mc_text_source &s, char *d_dst, char *last_byte = nullptr) {
        if (s.path) return file(s.path, s.n_bytes, d_dst, last_byte);
        if (last_byte && s.n_bytes > 0) *last_byte = s.text[s.n_bytes - 1];
        return text(s.text, s.n_bytes, d_dst);
    }
    int pad_and_wait(char *d_end) {              // 64 zero bytes behind a buffer's texts; everything sent is there
        HIP_TRY(hipMemsetAsync(d_end, 0, 64, c->up_stream));
        HIP_TRY(hipStreamSynchronize(c->up_stream));
        return 0;
    }
    // Two texts in one buffer, padded and waited for: the first, a newline if a second follows and the first lacked its last (its
    // last line ends where the second's first begins), the second (null: none) from *off2 on.  Room: both texts, 1 + 64 bytes
    int put_pair(const mc_text_source &s1, const mc_text_source *s2, char *d_dst, int64_t *off2) {
        char last1 = '\n';
        if (int rc = send(s1, d_dst, &last1)) return rc;
        *off2 = s1.n_bytes;
        if (s2 && s1.n_bytes > 0 && last1 != '\n') {
            HIP_TRY(hipMemsetAsync(d_dst + *off2, '\n', 1, c->up_stream));
            ++*off2;
        }
        if (s2)
            if (int rc = send(*s2, d_dst + *off2)) return rc;
        return pad_and_wait(d_dst + *off2 + (s2 ? s2->n_bytes : 0));
    }
    int put(Pool &pool, const mc_text_source &s, char **d_text) {  // one text in a buffer of its own, padded and waited for
        if (pool.get(d_text, (size_t)s.n_bytes + 64)) return -10;
        if (int rc = send(s, *d_text)) return rc;
        return pad_and_wait(*d_text + s.n_bytes);
    }
    template <typename S>
    void times(S &stats, std::chrono::steady_clock::time_point t0) const {             // ms_h2d: what the copies added behind the reads they ran beside
        stats.ms_read = ms_read;
        stats.ms_h2d = ms_since(t0) - ms_read;
    }
};

// ---- the frame of a call ----
// what a call owns while it runs: its device allocations, freed when the frame is left, and the feed its texts go through
struct Call {
    Pool pool;
    TextFeed feed;
    const std::chrono::steady_clock::time_point t0;
};

// One call of a file pipeline around its `body`: int(Call &), which returns 0 with the results filled in, 0 behind a decline (the
// status set) or an error.  blank(): the entry point's results to none -- run before the body, and behind it unless the call
// produced a result
template <typename S, typename Blank, typename Body>
int pipeline_call(mc_ctx *c, S &stats, int32_t *status, const char *who, size_t max_block, Blank blank, Body body) {
    blank();
    *status = 0;
    HIP_TRY(hipSetDevice(c->device));
    Call K{Pool(who), TextFeed(c, max_block), std::chrono::steady_clock::now()};
    stats = S();
    stats.decline_line = -1;
    const int rc = body(K);
    (void)hipStreamSynchronize(c->stream);                   // (whatever the way out: nothing of the pool is in use when it goes)
    if (rc != 0 || *status != 0) blank();
    stats.ms_total = ms_since(K.t0);
    return rc;
}

// mc_<pipeline>_last_stats: a copy of one of the pipeline's stats
template <typename P, typename S>
int stats_out(const char *what, mc_ctx *c, S *out, P mc_ctx::*pipe, S P::*member) {
    if (!c || !out) { mc_set_error("%s: bad arguments", what); return -12; }
    *out = (c->*pipe).*member;
    return 0;
}

// mc_<pipeline>_release: what the pipeline hands out and the feed's stages, behind everything that may still use them
template <typename P>
int release_pipeline(mc_ctx *c, P mc_ctx::*pipe) {
    if (!c) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    (c->*pipe).release();
    c->text_stages.release();
    return 0;
}

// A result of n bytes on the device into the pipeline's pinned block, waited for and handed out (n == 0: no block, no copy, a
// null pointer)
inline int fetch_out(mc_ctx *c, Grown &dst, const char *d_src, size_t n, const char **out, int64_t *n_out) {
    *out = nullptr; *n_out = 0;
    if (n == 0) return 0;
    if (int rc = dst.need(n)) return rc;
    HIP_TRY(hipMemcpyAsync(dst.get<char>(), d_src, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = dst.get<char>();
    *n_out = (int64_t)n;
    return 0;
}

}  // namespace
