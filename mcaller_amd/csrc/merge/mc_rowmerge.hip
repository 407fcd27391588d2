// mc_rowmerge.hip -- the merge behind `-t N` on the GPU: what mCaller.merge_like_sort_uniq writes for the part files of a run, the
// reference's `sort -n -k2 | uniq` (C ABI: mc_rows_merge_files / _text, mc_rows_merge_last_stats, mc_rows_merge_release; Python:
// Device.merge_rows, mCaller.merge_like_sort_uniq_device).  The unit stands in csrc/merge/, beside the units of the passes like
// csrc/bed/ and csrc/train/: no pass runs its kernels, and the benchmark's kernel hash names the files of the pass path one by one.
//
// The order is the host function's, not sort(1)'s: lines are bytes.splitlines(True) pieces (each with its '\n'), the key is
// (numeric prefix of field 2 as Decimal compares it, the bytes of the whole line, unsigned, the newline taking part), equal lines
// are written once.  No line is a proper prefix of another ('\n' occurs only at the end), so a line may be read as if zeros stood
// behind its newline.  The bytes are the host's, or the call declines and the host code does the files (status 1, mc_last_error):
//   * a '\r' anywhere (bytes.splitlines cuts there)
//   * a part file whose last byte is not '\n' (an empty file is fine)
//   * a numeric prefix with more than 18 significant integer digits or 18 fraction digits (mc_sortkey.h)
//   * a line longer than 65535 bytes (lengths are 16 bits)
//   * 2^31 - 2 lines or more (lines and places are numbered in 32 bits)
//   * texts that do not fit into free device memory beside the output and the tables: ALL texts stay resident, one behind the other
// Bytes >= 0x80 and control bytes other than '\r' compare as unsigned bytes: in scope.
//
// The steps (one lane per line or item unless said otherwise; n = lines):
//   kp_count / kp_scan / kp_starts   line starts (the device parser's kernels: mc_lines.h, launched by mc_textfeed.h)
//   km_cr         the smallest offset of a '\r', 16 bytes a load (atomicMin: whatever the order)
//   km_key        mc_sortkey.h on the line -> the 128-bit key (hi, lo), the length; a flagged line: line_flag (mc_textdev.h)
// then rounds over the ITEMS, the lines whose place is not yet decided (at first all of them, one segment).  A round orders every
// segment by one 64-bit word: the key's hi, the key's lo, then bytes [8r, 8r + 8) of the line, big-endian, zeros behind the newline:
//   km_word       the word of every item; OR and AND of all words and of all segment numbers (atomicOr / atomicAnd): a byte in which
//                 the two agree is the same in every item, and the host leaves its pass out
//   km_differs    does any segment hold two different words?  If none does the order stands and the round sorts nothing
//   km_count / kp_scan / km_scatter   a stable LSD radix sort over (segment, word), 8 bits a pass: digit counts per workgroup of
//                 4096 items, an exclusive scan over (digit, workgroup) in a launch of its own, a scatter chunk by chunk of 256 items
//                 with the in-workgroup stable ranks from ballots (as kb_sort_large, bed/mc_bedsum.hip)
//   km_heads      a new segment begins where (segment, word) differs from the item before; an item that equals it in a word that
//                 holds the newline is a duplicate: dropped (uniq).  Every item's line goes to its place in the permutation
//   km_segs / km_select / km_compact   segment numbers and sizes by a scan; a segment of one is done, one of up to 32 goes onto the
//                 list of km_small, the others' items (without the duplicates) are the next round's
//                 (the round of the key's hi word lists none: the lo word has yet to look at its ties)
//   km_small      a lane per listed segment: insertion sort by (lo, the bytes from the round's end on), duplicates dropped
// and the output: km_outlen / kp_scan / km_outoff (lengths of the kept lines in final order, scanned), km_gather (a wave per line).
// Rounds are bounded by the longest line; every kernel runs to its end alone; what crosses workgroups is a separate launch or an
// integer atomic (min, or, and, add to a counter; the list of km_small is worked through segment by segment, so its order does not
// matter).  wave64; no library sort; every buffer, event and stream through the owners of mc_own.h.
// The host side around the kernels -- a file's way onto the device through the context's two pinned stages, the line starts, the
// head's way back, the decline, the clock -- is mc_textfeed.h's, shared with the other units that take a whole text file.
#include "../mc_textfeed.h"
#include "../mc_sortkey.h"

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <string>

namespace {

constexpr int MG_SMALL = 32;                 // segments up to this size are finished by comparison
constexpr int MG_CHUNK = 4096;               // items a workgroup of a radix pass counts and scatters
constexpr int MG_MAX_LINE = 65535;
enum { MG_HI = 0, MG_LO = 1, MG_TEXT = 2 };
constexpr uint8_t MG_F_HEAD = 1, MG_F_DUP = 2, MG_F_STAY = 4;

struct MgHead {                              // device-side result block (copied to the host as it is)
    KpHead kp;                               // n_newlines (kp_scan), n_lines (kp_starts)
    unsigned long long decline;              // min over the flagged lines of line << 8 | reason (~0: none)
    unsigned long long cr_at;                // smallest offset of a '\r' (~0: none)
    unsigned long long w_or, w_and;          // over the round's words
    unsigned int s_or, s_and;                // over the round's segment numbers
    unsigned int n_small, largest_small;
    unsigned int differs, pad;               // some segment of the round holds two different words
    unsigned long long n_tied;               // items of the round in a segment of two or more
    long long n_seg, n_stay, n_out_bytes, n_kept, scratch;   // totals of the scans
};

struct MgArgs {
    const char *text;
    int64_t n_bytes, n_lines;
    const long long *line_start;
    MgHead *head;
    // per line
    uint64_t *khi, *klo;
    uint16_t *len;
    // per place in the final order
    uint32_t *perm;
    uint8_t *drop;
    long long *out_off;
    // per item: what a pass reads (src) and writes (dst); the places of the items (fixed during a round)
    uint64_t *kw, *kw_dst;
    uint32_t *sg, *sg_dst, *ln, *ln_dst, *apos, *apos_dst;
    uint8_t *fl;
    uint32_t *so, *seg_first, *small;
    long long *blk_sum, *blk_off;            // [2 * nblk] each
    long long *cnt, *cnt_off;                // [256 * workgroups of a pass] each
    char *out;
};

// bit 7 of every byte of v that equals '\r'
__device__ __forceinline__ uint32_t mg_cr_bits(uint32_t v) {
    v ^= 0x0D0D0D0Du;
    const uint32_t t = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | v | 0x7F7F7F7Fu);
}

// (the text buffer is padded with zeros: whole 16-byte groups are readable)
__global__ __launch_bounds__(256) void km_cr(const char *__restrict__ text, int64_t n, MgHead *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * 256 * 16;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16; i < n; i += stride) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + i);
        if (mg_cr_bits(v.x) | mg_cr_bits(v.y) | mg_cr_bits(v.z) | mg_cr_bits(v.w)) {
            for (int k = 0; k < 16; ++k)
                if (i + k < n && text[i + k] == '\r') { atomicMin(&head->cr_at, (unsigned long long)(i + k)); break; }
        }
    }
}

__global__ __launch_bounds__(256) void km_key(MgArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines) return;
    const int64_t b = A.line_start[li], e = A.line_start[li + 1];       // (every line has its newline: the host saw to it)
    uint64_t hi = 0, lo = 0;
    int len = 0;
    if (e - b > MG_MAX_LINE) line_flag(&A.head->decline, li, MC_MERGE_DECLINE_LONG_LINE);
    else {
        len = (int)(e - b);
        if (sk_key(reinterpret_cast<const unsigned char *>(A.text + b), len, &hi, &lo)) line_flag(&A.head->decline, li, MC_MERGE_DECLINE_KEY);
    }
    A.khi[li] = hi; A.klo[li] = lo; A.len[li] = (uint16_t)len;
    A.ln[li] = (uint32_t)li; A.sg[li] = 0u; A.apos[li] = (uint32_t)li;
    A.perm[li] = (uint32_t)li; A.drop[li] = 0;
}

__global__ void km_round_init(MgHead *head) {
    head->w_or = 0ull; head->w_and = ~0ull; head->s_or = 0u; head->s_and = ~0u;
    head->n_small = 0u; head->n_tied = 0ull; head->differs = 0u;
}

// bytes [off, off + 8) of line l, big-endian, zeros behind its end
__device__ __forceinline__ uint64_t mg_text_word(const MgArgs &A, uint32_t l, int off) {
    const unsigned char *t = reinterpret_cast<const unsigned char *>(A.text) + A.line_start[l];
    const int len = A.len[l];
    uint64_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w = (w << 8) | (uint64_t)(off + k < len ? t[off + k] : 0u);
    return w;
}

__global__ __launch_bounds__(256) void km_word(MgArgs A, int64_t m, int kind, int off) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long w_or = 0ull, w_and = ~0ull;
    unsigned int s_or = 0u, s_and = ~0u;
    if (j < m) {
        const uint32_t l = A.ln[j];
        const uint64_t w = kind == MG_HI ? A.khi[l] : kind == MG_LO ? A.klo[l] : mg_text_word(A, l, off);
        A.kw[j] = w;
        w_or = w_and = w;
        s_or = s_and = A.sg[j];
    }
    for (int o = 32; o > 0; o >>= 1) {
        w_or |= __shfl_xor(w_or, o); w_and &= __shfl_xor(w_and, o);
        s_or |= __shfl_xor(s_or, o); s_and &= __shfl_xor(s_and, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&A.head->w_or, w_or); atomicAnd(&A.head->w_and, w_and);
        atomicOr(&A.head->s_or, s_or); atomicAnd(&A.head->s_and, s_and);
    }
}

// is there a segment whose items differ in the round's word?  (where a read's rows share the next 8 bytes of the name there is
// not, whatever the other reads' names are: the order stands and the round sorts nothing)
__global__ __launch_bounds__(256) void km_differs(MgArgs A, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool d = j > 0 && j < m && A.sg[j] == A.sg[j - 1] && A.kw[j] != A.kw[j - 1];
    if (__ballot(d) && (threadIdx.x & 63) == 0) atomicOr(&A.head->differs, 1u);
}

__device__ __forceinline__ unsigned mg_digit(const MgArgs &A, int64_t j, int of_seg, int sh) {
    return of_seg ? (A.sg[j] >> sh) & 255u : (unsigned)(A.kw[j] >> sh) & 255u;
}

// cnt[digit * workgroups + workgroup]: items of the workgroup's chunk with that digit
__global__ __launch_bounds__(256) void km_count(MgArgs A, int64_t m, int of_seg, int sh) {
    __shared__ unsigned s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * MG_CHUNK;
    for (int i = threadIdx.x; i < MG_CHUNK; i += 256)
        if (c0 + i < m) atomicAdd(&s_hist[mg_digit(A, c0 + i, of_seg, sh)], 1u);
    __syncthreads();
    A.cnt[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (long long)s_hist[threadIdx.x];
}

// The scatter goes chunk by chunk of 256 items in order and is stable: an item's place = the digit's base + items of that digit in
// earlier waves of the chunk + those before it in its wave
__global__ __launch_bounds__(256) void km_scatter(MgArgs A, int64_t m, int of_seg, int sh) {
    __shared__ long long s_base[256];
    __shared__ unsigned s_wc[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = A.cnt_off[(size_t)tid * gridDim.x + blockIdx.x];
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * MG_CHUNK;
    for (int s0 = 0; s0 < MG_CHUNK && c0 + s0 < m; s0 += 256) {
        const int64_t j = c0 + s0 + tid;
        const bool valid = j < m;
        const unsigned d = valid ? mg_digit(A, j, of_seg, sh) : 0u;
        unsigned long long peers = __ballot(valid);             // lanes of the wave with an item of the same digit
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(one);
            peers &= one ? bal : ~bal;
        }
        const unsigned before_me = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        const bool leader = valid && before_me == 0;
        for (int w = 0; w < 4; ++w) s_wc[w][tid] = 0;
        __syncthreads();
        if (leader) s_wc[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (valid) {
            long long at = s_base[d] + before_me;
            for (int w = 0; w < wave; ++w) at += s_wc[w][d];
            A.kw_dst[at] = A.kw[j]; A.sg_dst[at] = A.sg[j]; A.ln_dst[at] = A.ln[j];
        }
        __syncthreads();
        if (leader) atomicAdd((unsigned long long *)&s_base[d], (unsigned long long)__popcll(peers));
        __syncthreads();
    }
}

// exclusive prefix of v over the workgroup's 256 threads; *total: the workgroup's sum
__device__ __forceinline__ long long mg_block_excl(long long v, long long *s_w, long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    __syncthreads();
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    long long before = 0;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before + incl - v;
}

__global__ __launch_bounds__(256) void km_heads(MgArgs A, int64_t m, int kind, int off) {
    __shared__ long long s_w[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    if (j < m) {
        const uint32_t l = A.ln[j];
        head = j == 0 || A.sg[j] != A.sg[j - 1] || A.kw[j] != A.kw[j - 1];
        // equal to the item before in a word that holds the newline: the same line (nothing stands behind a newline)
        const bool dup = !head && kind == MG_TEXT && off + 8 >= (int)A.len[l];
        A.fl[j] = (uint8_t)((head ? MG_F_HEAD : 0) | (dup ? MG_F_DUP : 0));
        const uint32_t p = A.apos[j];
        A.perm[p] = l;
        if (dup) A.drop[p] = 1;
    }
    long long tot;
    (void)mg_block_excl(head ? 1 : 0, s_w, &tot);
    if (threadIdx.x == 0) A.blk_sum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void km_segs(MgArgs A, int64_t m) {
    __shared__ long long s_w[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool head = j < m && (A.fl[j] & MG_F_HEAD);
    long long tot;
    const long long s = A.blk_off[blockIdx.x] + mg_block_excl(head ? 1 : 0, s_w, &tot) + (head ? 1 : 0) - 1;
    if (j < m) {
        A.so[j] = (uint32_t)s;
        if (head) A.seg_first[s] = (uint32_t)j;
        if (j == m - 1) A.seg_first[s + 1] = (uint32_t)m;
    }
}

// small_max: segments of 2 .. small_max items go onto the list of km_small (1: none -- the round of the key's hi word, whose ties
// the lo word has yet to look at)
__global__ __launch_bounds__(256) void km_select(MgArgs A, int64_t m, int64_t nblk, uint32_t small_max) {
    __shared__ long long s_w[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool stay = false, tied = false;
    if (j < m) {
        const uint32_t s = A.so[j];
        const uint32_t size = A.seg_first[s + 1] - A.seg_first[s];
        const uint8_t fl = A.fl[j];
        tied = size >= 2u;
        stay = size > small_max && !(fl & MG_F_DUP);
        if ((fl & MG_F_HEAD) && size >= 2u && size <= small_max) {
            A.small[atomicAdd(&A.head->n_small, 1u)] = (uint32_t)j;
            atomicMax(&A.head->largest_small, size);
        }
        A.fl[j] = (uint8_t)(fl | (stay ? MG_F_STAY : 0));
    }
    const unsigned long long bal = __ballot(tied);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_tied, (unsigned long long)__popcll(bal));
    long long tot;
    (void)mg_block_excl(stay ? 1 : 0, s_w, &tot);
    if (threadIdx.x == 0) A.blk_sum[nblk + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void km_compact(MgArgs A, int64_t m, int64_t nblk) {
    __shared__ long long s_w[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool stay = j < m && (A.fl[j] & MG_F_STAY);
    long long tot;
    const long long t = A.blk_off[nblk + blockIdx.x] + mg_block_excl(stay ? 1 : 0, s_w, &tot);
    if (stay) { A.ln_dst[t] = A.ln[j]; A.apos_dst[t] = A.apos[j]; A.sg_dst[t] = A.so[j]; }
}

// lines a and b, which agree in their first `off` bytes (and in the key's hi word): -1, 0, 1 by (lo, the bytes)
__device__ __forceinline__ int mg_compare(const MgArgs &A, uint32_t a, uint32_t b, int off) {
    const uint64_t la = A.klo[a], lb = A.klo[b];
    if (la != lb) return la < lb ? -1 : 1;
    const unsigned char *ta = reinterpret_cast<const unsigned char *>(A.text) + A.line_start[a];
    const unsigned char *tb = reinterpret_cast<const unsigned char *>(A.text) + A.line_start[b];
    const int na = A.len[a], nb = A.len[b], n = min(na, nb);
    for (int i = off; i < n; ++i)
        if (ta[i] != tb[i]) return ta[i] < tb[i] ? -1 : 1;
    return na == nb ? 0 : na < nb ? -1 : 1;      // (lengths differ only where a line ended before `off`: never among tied lines)
}

__global__ __launch_bounds__(256) void km_small(MgArgs A, unsigned n_small, int off) {
    const unsigned q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_small) return;
    const uint32_t first = A.small[q];
    const uint32_t s = A.so[first];
    const uint32_t size = A.seg_first[s + 1] - first;
    uint32_t *b = A.ln + first;
    for (uint32_t i = 1; i < size; ++i) {
        const uint32_t v = b[i];
        uint32_t k = i;
        for (; k > 0 && mg_compare(A, b[k - 1], v, off) > 0; --k) b[k] = b[k - 1];
        b[k] = v;
    }
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t p = A.apos[first + i];
        A.perm[p] = b[i];
        A.drop[p] = (uint8_t)(i > 0 && mg_compare(A, b[i - 1], b[i], off) == 0);
    }
}

__device__ __forceinline__ long long mg_out_len(const MgArgs &A, int64_t p) {
    return p < A.n_lines && !A.drop[p] ? (long long)A.len[A.perm[p]] : 0;
}

__global__ __launch_bounds__(256) void km_outlen(MgArgs A, int64_t nblk) {
    __shared__ long long s_w[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool kept = p < A.n_lines && !A.drop[p];
    long long tot_b, tot_k;
    (void)mg_block_excl(mg_out_len(A, p), s_w, &tot_b);
    (void)mg_block_excl(kept ? 1 : 0, s_w, &tot_k);
    if (threadIdx.x == 0) { A.blk_sum[blockIdx.x] = tot_b; A.blk_sum[nblk + blockIdx.x] = tot_k; }
}

__global__ __launch_bounds__(256) void km_outoff(MgArgs A) {
    __shared__ long long s_w[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    long long tot;
    const long long at = A.blk_off[blockIdx.x] + mg_block_excl(mg_out_len(A, p), s_w, &tot);
    if (p < A.n_lines) A.out_off[p] = at;
}

// a wave per place: the kept line's bytes to their offset
__global__ __launch_bounds__(256) void km_gather(MgArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= A.n_lines || A.drop[p]) return;
    const uint32_t l = A.perm[p];
    const char *src = A.text + A.line_start[l];
    char *dst = A.out + A.out_off[p];
    const int len = A.len[l];
    for (int i = lane; i < len; i += 64) dst[i] = src[i];
}

const char *mg_reason_text(int reason) {
    switch (reason) {
    case MC_MERGE_DECLINE_CR: return "a carriage return (bytes.splitlines cuts there)";
    case MC_MERGE_DECLINE_NO_NEWLINE: return "a part file that does not end in a newline";
    case MC_MERGE_DECLINE_KEY: return "a numeric prefix of field 2 with more than 18 integer or 18 fraction digits";
    case MC_MERGE_DECLINE_LONG_LINE: return "a line longer than 65535 bytes";
    case MC_MERGE_DECLINE_ROWS: return "more lines than are numbered (2^31 - 2)";
    case MC_MERGE_DECLINE_MEMORY: return "the texts, the output and the tables do not fit into free device memory";
    }
    return "unknown";
}

// the part files' texts, one behind the other: file i is bytes [end[i - 1], end[i])
struct MgFiles { std::vector<int64_t> end; };

int mg_file_of(const MgFiles &F, int64_t offset) {
    for (size_t i = 0; i < F.end.size(); ++i)
        if (offset < F.end[i]) return (int)i;
    return -1;
}

int mg_decline(mc_ctx *c, int32_t *status, int reason, long long line, int file) {
    c->mg.stats.decline_file = file;
    return decline(c->mg.stats, status, "merge", mg_reason_text(reason), reason, line);
}

constexpr size_t MG_BYTES_PER_LINE = 8 + 8 + 8 + 2 + 4 + 1 + 8 + 2 * (8 + 4 + 4 + 4) + 1 + 4 + 4 + 4 + 4;   // the tables of MgArgs

// one radix pass over the m items: 8 bits of the word (of_seg = 0) or of the segment number at shift sh
int mg_pass(mc_ctx *c, MgArgs &A, int64_t m, int of_seg, int sh) {
    hipStream_t st = c->stream;
    const unsigned wgs = (unsigned)((m + MG_CHUNK - 1) / MG_CHUNK);
    hipLaunchKernelGGL(km_count, dim3(wgs), dim3(256), 0, st, A, m, of_seg, sh);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.cnt, (int64_t)256 * wgs, A.cnt_off, &A.head->scratch);
    hipLaunchKernelGGL(km_scatter, dim3(wgs), dim3(256), 0, st, A, m, of_seg, sh);
    std::swap(A.kw, A.kw_dst); std::swap(A.sg, A.sg_dst); std::swap(A.ln, A.ln_dst);
    c->mg.stats.n_passes += 1;
    c->mg.stats.kernel_bytes += m * (of_seg ? 4 : 8) + m * 2 * 16 + (int64_t)wgs * 256 * 8 * 4;
    return 0;
}

// a call of either entry point: the texts one behind the other on the device (mg_upload), and what mg_run makes of them
struct MgCall {
    MgFiles F;
    char *d_text = nullptr;
    int64_t n = 0;                               // bytes of all texts
    int64_t bad_end = -1;                        // the offset behind the first part file that does not end in a newline, -1: none
    size_t block = 0;                            // the step the output leaves in (mc_rows_merge_files)
    MgArgs A = {};                               // A.out: the output on the device ...
    int64_t nb = 0;                              // ... and its bytes
};

// The texts are on the device (d_text[0, n), padded; copies enqueued on c->up_stream): everything up to the output in A.out.
// bad_end: the offset behind a part file that does not end in a newline, -1: none
int mg_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const MgFiles &F, int64_t bad_end, MgArgs &A, int64_t *n_out,
           int32_t *status) {
    mc_rows_merge_stats &S = c->mg.stats;
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    const auto t_kernels = std::chrono::steady_clock::now();
    *n_out = 0;
    if (n == 0) return 0;
    MgHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline = ~0ull; h.cr_at = ~0ull;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    long long *tile_off = nullptr, *line_start = nullptr;
    if (int rc = lines_count(pool, st, d_text, n, &d_head->kp, &tile_off)) return rc;
    hipLaunchKernelGGL(km_cr, dim3((unsigned)std::min<int64_t>((n + 4095) / 4096, 8192)), dim3(256), 0, st, d_text, n, d_head);
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.kernel_bytes += 2 * n;
    const int64_t n_nl = h.kp.n_newlines;
    if (too_many_lines(n_nl)) return mg_decline(c, status, MC_MERGE_DECLINE_ROWS, -1, -1);
    if (!device_fits((size_t)(n_nl + 2) * MG_BYTES_PER_LINE + (size_t)n + ((size_t)4 << 20))) return mg_decline(c, status, MC_MERGE_DECLINE_MEMORY, -1, -1);
    if (int rc = lines_starts(pool, st, d_text, n, n_nl, tile_off, &d_head->kp, &line_start)) return rc;
    S.kernel_bytes += n + n_nl * 8;
    // a '\r' or a file without its last newline: the first of them, and the line it lies in (the starts are fetched for that alone)
    int64_t bad_at = -1;
    int bad_reason = 0;
    if (bad_end >= 0) { bad_at = bad_end - 1; bad_reason = MC_MERGE_DECLINE_NO_NEWLINE; }
    if (h.cr_at != ~0ull && (bad_at < 0 || (int64_t)h.cr_at < bad_at)) { bad_at = (int64_t)h.cr_at; bad_reason = MC_MERGE_DECLINE_CR; }
    if (bad_at >= 0) {
        std::vector<long long> starts((size_t)n_nl + 1);
        HIP_TRY(hipMemcpyAsync(starts.data(), line_start, starts.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const long long line = (long long)(std::upper_bound(starts.begin(), starts.end(), (long long)bad_at) - starts.begin()) - 1;
        return mg_decline(c, status, bad_reason, line, mg_file_of(F, bad_at));
    }
    const int64_t n_lines = n_nl;                             // (every file ends in a newline, so the text does)
    S.n_lines = n_lines;
    if (n_lines == 0) return 0;
    const size_t nl = (size_t)n_lines;
    const int64_t nblk = (n_lines + 255) / 256;
    const size_t pass_wgs = (size_t)((n_lines + MG_CHUNK - 1) / MG_CHUNK);
    A.text = d_text; A.n_bytes = n; A.n_lines = n_lines; A.line_start = line_start; A.head = d_head;
    if (pool.get(&A.khi, nl) || pool.get(&A.klo, nl) || pool.get(&A.len, nl) || pool.get(&A.perm, nl) || pool.get(&A.drop, nl) ||
        pool.get(&A.out_off, nl) || pool.get(&A.kw, nl) || pool.get(&A.kw_dst, nl) || pool.get(&A.sg, nl) || pool.get(&A.sg_dst, nl) ||
        pool.get(&A.ln, nl) || pool.get(&A.ln_dst, nl) || pool.get(&A.apos, nl) || pool.get(&A.apos_dst, nl) || pool.get(&A.fl, nl) ||
        pool.get(&A.so, nl) || pool.get(&A.seg_first, nl + 1) || pool.get(&A.small, nl) || pool.get(&A.blk_sum, (size_t)2 * nblk) ||
        pool.get(&A.blk_off, (size_t)2 * nblk) || pool.get(&A.cnt, 256 * pass_wgs) || pool.get(&A.cnt_off, 256 * pass_wgs))
        return -10;
    const unsigned lb = (unsigned)nblk;
    hipLaunchKernelGGL(km_key, dim3(lb), dim3(256), 0, st, A);
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.kernel_bytes += n_lines * (8 + 60 + 8 + 8 + 2 + 4 * 4 + 1);       // the starts, the bytes up to the key's end, the columns
    if (h.decline != ~0ull) {
        const long long line = decline_line(h.decline);
        long long at = 0;
        HIP_TRY(hipMemcpy(&at, line_start + line, 8, hipMemcpyDeviceToHost));
        return mg_decline(c, status, decline_reason(h.decline), line, mg_file_of(F, at));
    }
    // the rounds
    int64_t m = n_lines;
    int kind = MG_HI, off = 0;
    while (m > 0) {
        if (off > MG_MAX_LINE + 8) { mc_set_error("the device merge: lines still tied behind their end"); return -11; }
        const unsigned mb = (unsigned)((m + 255) / 256);
        const int64_t mblk = mb;
        hipLaunchKernelGGL(km_round_init, dim3(1), dim3(1), 0, st, d_head);
        hipLaunchKernelGGL(km_word, dim3(mb), dim3(256), 0, st, A, m, kind, off);
        hipLaunchKernelGGL(km_differs, dim3(mb), dim3(256), 0, st, A, m);
        if (int rc = fetch_head(st, d_head, h)) return rc;
        S.kernel_bytes += m * (4 + 8 + 4 + (kind == MG_TEXT ? 8 + 2 + 8 : 8)) + m * 12;
        const uint64_t diff_w = h.w_or ^ h.w_and;
        const uint32_t diff_s = h.s_or ^ h.s_and;
        if (h.differs) {                                      // (no segment with two different words: the order stands)
            for (int b = 0; b < 8; ++b)
                if ((diff_w >> (8 * b)) & 255u)
                    if (int rc = mg_pass(c, A, m, 0, 8 * b)) return rc;
            for (int b = 0; b < 4; ++b)
                if ((diff_s >> (8 * b)) & 255u)
                    if (int rc = mg_pass(c, A, m, 1, 8 * b)) return rc;
        }
        const int off_next = kind == MG_TEXT ? off + 8 : 0;
        hipLaunchKernelGGL(km_heads, dim3(mb), dim3(256), 0, st, A, m, kind, off);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.blk_sum, mblk, A.blk_off, &d_head->n_seg);
        hipLaunchKernelGGL(km_segs, dim3(mb), dim3(256), 0, st, A, m);
        hipLaunchKernelGGL(km_select, dim3(mb), dim3(256), 0, st, A, m, mblk, kind == MG_HI ? 1u : (uint32_t)MG_SMALL);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)(A.blk_sum + mblk), mblk, A.blk_off + mblk, &d_head->n_stay);
        hipLaunchKernelGGL(km_compact, dim3(mb), dim3(256), 0, st, A, m, mblk);
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.n_small > 0)
            hipLaunchKernelGGL(km_small, dim3((h.n_small + 255) / 256), dim3(256), 0, st, A, h.n_small, off_next);
        HIP_TRY(hipGetLastError());
        S.kernel_bytes += m * (2 * 12 + 4 + 2 + 4 + 1 + 4 + 1 + 4 + 8 + 1 + 1 + 4 + 1) + h.n_stay * 12 + (int64_t)h.n_tied * 0;
        S.n_rounds += 1;
        if (kind == MG_LO) S.n_tied_after_key = (int64_t)h.n_tied;
        // what stays: in the other set of columns (the places with them); km_small sorted the old set in place
        std::swap(A.ln, A.ln_dst); std::swap(A.sg, A.sg_dst); std::swap(A.apos, A.apos_dst);
        m = h.n_stay;
        if (kind == MG_TEXT) off += 8;
        else kind += 1;
    }
    S.largest_compared = (int32_t)h.largest_small;
    // the output
    hipLaunchKernelGGL(km_outlen, dim3(lb), dim3(256), 0, st, A, nblk);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.blk_sum, nblk, A.blk_off, &d_head->n_out_bytes);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)(A.blk_sum + nblk), nblk, A.blk_off + nblk, &d_head->n_kept);
    hipLaunchKernelGGL(km_outoff, dim3(lb), dim3(256), 0, st, A);
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.n_lines_out = h.n_kept;
    S.n_out_bytes = h.n_out_bytes;
    if (h.n_out_bytes > 0) {
        if (!device_fits((size_t)h.n_out_bytes)) return mg_decline(c, status, MC_MERGE_DECLINE_MEMORY, -1, -1);
        if (pool.get(&A.out, (size_t)h.n_out_bytes)) return -10;
        hipLaunchKernelGGL(km_gather, dim3((unsigned)((n_lines + 3) / 4)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    S.kernel_bytes += 2 * n_lines * (1 + 4 + 2) + n_lines * (8 + 1 + 4 + 8 + 8 + 2) + 2 * h.n_out_bytes;
    S.ms_kernels = ms_since(t_kernels);
    *n_out = h.n_out_bytes;
    return 0;
}

// what both entry points begin with: the sources' texts onto the device, one behind the other -> 0: go on; 1: done (declined,
// *status set); < 0: an error
int mg_upload(mc_ctx *c, Call &K, MgCall &M, const mc_text_source *src, int n_src, int32_t *status) {
    TextFeed &feed = K.feed;
    for (int i = 0; i < n_src; ++i) M.F.end.push_back(M.n += src[i].n_bytes);
    c->mg.stats.decline_file = -1;
    c->mg.stats.n_bytes = M.n;
    if (!device_fits(2 * (size_t)M.n + 4096)) { (void)mg_decline(c, status, MC_MERGE_DECLINE_MEMORY, -1, -1); return 1; }
    if (K.pool.get(&M.d_text, (size_t)M.n + 64)) return -10;
    M.block = feed.block_for(M.n);
    // files (a call's sources are all files or all texts): the stages sized once, before the first block, for the step of all
    // texts together -- the output's
    if (n_src > 0 && src[0].path)
        if (int rc = feed.stages(M.block)) return rc;
    for (int i = 0; i < n_src; ++i) {
        char last = '\n';
        if (int rc = feed.send(src[i], M.d_text + (M.F.end[i] - src[i].n_bytes), &last)) return rc;
        if (last != '\n' && M.bad_end < 0) M.bad_end = M.F.end[i];
    }
    if (int rc = feed.pad_and_wait(M.d_text + M.n)) return rc;
    feed.times(c->mg.stats, K.t0);
    return 0;
}

int mg_write_all(int fd, const char *p, size_t n) {
    while (n > 0) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            return -1;
        }
        p += w; n -= (size_t)w;
    }
    return 0;
}

// The output in blocks through the feed's two stages: a block is written while the next is on its way.  The file appears under
// its name only when it is complete
int mg_to_file(mc_ctx *c, const MgCall &M, const char *out_path) {
    int rc = 0;
    TextStages &T = c->text_stages;
    const int64_t nb = M.nb, cap = (int64_t)M.block;
    const std::string tmp = std::string(out_path) + ".merging";
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { mc_set_error("mc_rows_merge_files: cannot write %s: %s", tmp.c_str(), strerror(errno)); rc = -1; }
    double ms_write = 0;
    const auto t_out = std::chrono::steady_clock::now();
    // block i goes through stage i & 1: its successor is enqueued before block i is waited for and written
    const int64_t n_blocks_out = (nb + cap - 1) / cap;
    auto enqueue = [&](int64_t i) {
        const int64_t lo = i * cap, k = std::min<int64_t>(cap, nb - lo);
        int r = mc_hip_rc(hipMemcpyAsync(T.stage[i & 1].p, M.A.out + lo, (size_t)k, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
        if (r == 0) r = mc_hip_rc(hipEventRecord(T.ev[i & 1], c->stream), "hipEventRecord");
        return r;
    };
    if (rc == 0 && n_blocks_out > 0) rc = enqueue(0);
    for (int64_t i = 0; i < n_blocks_out && rc == 0; ++i) {
        if (i + 1 < n_blocks_out) rc = enqueue(i + 1);
        if (rc == 0) rc = mc_hip_rc(hipEventSynchronize(T.ev[i & 1]), "hipEventSynchronize");
        if (rc) break;
        const auto tw = std::chrono::steady_clock::now();
        if (mg_write_all(fd, T.stage[i & 1].get<char>(), (size_t)std::min<int64_t>(cap, nb - i * cap))) {
            mc_set_error("mc_rows_merge_files: writing %s failed: %s", tmp.c_str(), strerror(errno));
            rc = -1;
        }
        ms_write += ms_since(tw);
    }
    if (fd >= 0 && close(fd) != 0 && rc == 0) { mc_set_error("mc_rows_merge_files: closing %s failed: %s", tmp.c_str(), strerror(errno)); rc = -1; }
    if (rc == 0 && rename(tmp.c_str(), out_path) != 0) {
        mc_set_error("mc_rows_merge_files: renaming %s failed: %s", tmp.c_str(), strerror(errno));
        rc = -1;
    }
    if (rc != 0 && fd >= 0) (void)unlink(tmp.c_str());
    c->mg.stats.ms_write = ms_write;
    c->mg.stats.ms_d2h = ms_since(t_out) - ms_write;
    return rc;
}

}  // namespace

extern "C" int mc_rows_merge_text(mc_ctx *c, const char *text, int64_t n_bytes, const char **out, int64_t *n_out, int32_t *status) {
    if (!c || !out || !n_out || !status || n_bytes < 0 || (n_bytes > 0 && !text)) {
        mc_set_error("mc_rows_merge_text: bad arguments");
        return -12;
    }
    const mc_text_source src = {text, nullptr, n_bytes};
    MgCall M;
    return pipeline_call(c, c->mg.stats, status, "row merge", (size_t)64 << 20, [&] { *out = nullptr; *n_out = 0; }, [&](Call &K) -> int {
        if (int rc = mg_upload(c, K, M, &src, 1, status)) return rc < 0 ? rc : 0;
        if (int rc = mg_run(c, K.pool, M.d_text, M.n, M.F, M.bad_end, M.A, &M.nb, status)) return rc;
        if (*status != 0) return 0;
        const auto t_d2h = std::chrono::steady_clock::now();
        const int rc = fetch_out(c, c->mg.out, M.A.out, (size_t)M.nb, out, n_out);
        c->mg.stats.ms_d2h = ms_since(t_d2h);
        return rc;
    });
}

extern "C" int mc_rows_merge_files(mc_ctx *c, const char *const *paths, int32_t n_paths, const char *out_path, int64_t *n_lines_out,
                                   int32_t *status) {
    if (!c || !paths || n_paths < 0 || !out_path || !n_lines_out || !status) {
        mc_set_error("mc_rows_merge_files: bad arguments");
        return -12;
    }
    std::vector<mc_text_source> src((size_t)n_paths);
    for (int i = 0; i < n_paths; ++i) {
        src[i] = mc_text_source{nullptr, paths[i], 0};
        if (int rc = regular_file_size("mc_rows_merge_files", paths[i], &src[i].n_bytes)) return rc;
    }
    MgCall M;
    return pipeline_call(c, c->mg.stats, status, "row merge", (size_t)64 << 20, [&] { *n_lines_out = 0; }, [&](Call &K) -> int {
        if (int rc = mg_upload(c, K, M, src.data(), n_paths, status)) return rc < 0 ? rc : 0;
        if (int rc = mg_run(c, K.pool, M.d_text, M.n, M.F, M.bad_end, M.A, &M.nb, status)) return rc;
        if (*status != 0) return 0;
        if (int rc = mg_to_file(c, M, out_path)) return rc;
        *n_lines_out = c->mg.stats.n_lines_out;
        return 0;
    });
}

extern "C" int mc_rows_merge_last_stats(mc_ctx *c, mc_rows_merge_stats *out) {
    return stats_out("mc_rows_merge_last_stats", c, out, &mc_ctx::mg, &MergePipe::stats);
}

extern "C" int mc_rows_merge_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::mg); }
