// The eventalign text parsed ON THE GPU (included by mc_tables.hip; its line-start kernels also by mc_lines.h, see below; the kernels sit in an unnamed namespace; C ABI: mc_ctx_parse_begin / _end / _finish).
//
// What it replaces: the row ingest of the reference's loop, extract_contexts.py:140-152 -- `line.split()[:12]`, int(), float(),
// the two k-mer comparisons -- which mc_parse.cpp does on the host with every core the process may use.  On a GPU box the
// cores are the scarce part (this pool's containers get 16 CPUs' worth of time per 100 ms, cpu.max; parsing costs ~0.8 CPU
// seconds per GB of text), the link is not: the text goes over PCIe as it is (117 B/row instead of 17 B/row of columns) and
// the columns are made where they are needed.  The host only moves the bytes (pread into pinned memory) and keeps the
// strings: read names -> read ids -> qualities, contig names, messages.
//
//   kp_count / kp_scan / kp_starts   line starts: newlines per 16 KB tile, exclusive scan, one pass that writes the offsets
//   kp_parse                          one lane per line: the first 12 whitespace-separated tokens (str.split()'s ASCII
//                                     whitespace), contig -> id through a hash table of the reference's names, int(), the
//                                     plain-decimal float form (<= 9 integer, <= 4 fractional digits) as units of 1e-4,
//                                     reference_kmer == model_kmer, model_kmer == "NNNNNN"; line-indexed scratch columns
//   kp_count_rows / kp_scan / kp_place   rows = lines that are rows (>= 12 tokens, known contig), in order: the columns go to
//                                     their place in the table slot; a row whose read name differs from the row before it
//                                     starts a name block, a change of name or contig starts a segment (listed)
//
// Exactness: anything this path does not reproduce bit for bit is not attempted -- a token int()/float() would reject or
// that needs strtod (exponents, more digits, inf/nan), values out of range, more rows or segments than the slot holds --
// the line is flagged and the caller parses the shard with the host parser instead (which also words the reference's error
// messages).  tests/test_gpu_devparse.py compares every column with the host parser's on all fixtures and on random text.
//
// The line-start kernels serve a second unit, the summary of a .diffs file (bed/mc_bedsum.hip): it includes this file through
// mc_lines.h, which defines MC_LINES_ONLY -- everything below kp_starts is left out then.  The kernels' text stays here, one
// definition, in the file the benchmark's kernel hash covers.
namespace {

constexpr int KP_TILE = 16384, KP_THREADS = 256;           // bytes per tile of the newline passes: 64 per thread
#ifndef MC_LINES_ONLY
constexpr int KP_ST_ROW = 0, KP_ST_SKIP = 1, KP_ST_UNKNOWN = 2, KP_ST_HOST = 3;
constexpr int KP_MAX_UNKNOWN = 4096;
constexpr int KP_EAGER_SEGS = 4096, KP_EAGER_UNKNOWN = 64;   // what travels to the host with the head, unasked

// (the host-side structures KpHead, KpUnknown, KpScratch, KpContigs: mc_ctx.h; struct KpSeg: mc_dev.h)

__device__ __forceinline__ bool kp_is_ws(unsigned c) {      // ASCII subset of what str.split() treats as whitespace
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31);
}
#endif

// bit 7 of every byte of v that equals '\n'
__device__ __forceinline__ uint32_t kp_nl_bits(uint32_t v) {
    v ^= 0x0A0A0A0Au;
    const uint32_t t = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | v | 0x7F7F7F7Fu);
}

// newlines of the thread's 64 bytes [b, b + 64) of text[0, n)
__device__ __forceinline__ int kp_count64(const char *__restrict__ text, int64_t n, int64_t b) {
    int cnt = 0;
    if (b + 64 <= n) {
        const uint4 *p = reinterpret_cast<const uint4 *>(text + b);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = p[i];
            cnt += __popc(kp_nl_bits(v.x)) + __popc(kp_nl_bits(v.y)) + __popc(kp_nl_bits(v.z)) + __popc(kp_nl_bits(v.w));
        }
    } else {
        for (int64_t i = b; i < n; ++i) cnt += text[i] == '\n';
    }
    return cnt;
}

__global__ __launch_bounds__(KP_THREADS) void kp_count(const char *__restrict__ text, int64_t n, long long *__restrict__ tile_cnt) {
    __shared__ int s_w[KP_THREADS / 64];
    const int64_t b = (int64_t)blockIdx.x * KP_TILE + threadIdx.x * 64;
    int cnt = b < n ? kp_count64(text, n, b) : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (long long)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// exclusive scan of cnt[0, n) into off[0, n), the total into *total: one workgroup (n is a few ten thousand)
__global__ __launch_bounds__(1024) void kp_scan(const long long *__restrict__ cnt, int64_t n, long long *__restrict__ off,
                                                long long *__restrict__ total) {
    __shared__ long long s_w[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const long long c = i < n ? cnt[i] : 0;
        long long incl = c;
        for (int o = 1; o < 64; o <<= 1) {
            const long long v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        long long before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_w[w];
        if (i < n) off[i] = before + incl - c;
        __syncthreads();
        if (tid == 1023) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

// line_start[1 + j] = offset behind the j-th newline; line_start[0] = 0; the head's line count
__global__ __launch_bounds__(KP_THREADS) void kp_starts(const char *__restrict__ text, int64_t n, const long long *__restrict__ tile_off,
                                                        long long *__restrict__ line_start, int64_t cap_lines,
                                                        KpHead *__restrict__ head) {
    __shared__ int s_w[KP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x * KP_TILE + tid * 64;
    uint32_t m[16];                     // bit 7 of every newline byte, word by word (whole 64-byte pieces inside the text)
    int cnt = 0;
    const bool whole = b + 64 <= n;
    if (whole) {
        const uint4 *p = reinterpret_cast<const uint4 *>(text + b);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = p[i];
            m[4 * i] = kp_nl_bits(v.x); m[4 * i + 1] = kp_nl_bits(v.y); m[4 * i + 2] = kp_nl_bits(v.z); m[4 * i + 3] = kp_nl_bits(v.w);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) cnt += __popc(m[i]);
    } else if (b < n) {
        for (int64_t i = b; i < n; ++i) cnt += text[i] == '\n';
    }
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    long long at = tile_off[blockIdx.x] + incl - cnt;
    for (int w = 0; w < wave; ++w) at += s_w[w];
    if (cnt) {
        if (whole) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                uint32_t w = m[i];
                while (w) {
                    const int byte = (__ffs(w) - 1) >> 3;
                    w &= w - 1;
                    if (at + 1 < cap_lines) line_start[at + 1] = b + 4 * i + byte + 1;
                    ++at;
                }
            }
        } else {
            for (int64_t i = b; i < n; ++i)
                if (text[i] == '\n') {
                    if (at + 1 < cap_lines) line_start[at + 1] = i + 1;
                    ++at;
                }
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        line_start[0] = 0;
        const long long nl = head->n_newlines;
        const long long lines = n > 0 ? nl + (text[n - 1] != '\n' ? 1 : 0) : 0;
        head->n_lines = lines;
        if (lines + 1 > cap_lines) head->overflow |= 1;
    }
}

#ifndef MC_LINES_ONLY
// A copy done by the compute units instead of a DMA engine (host memory: pinned, so the GPU addresses it).  The DMA
// engines take transfers in the order they were submitted, whichever stream they came from: a 100 KB copy submitted while a
// 150 MB shard of text is on its way completes when the text has arrived, 2.8 ms later (measured) -- and every small transfer of
// the streaming path (the small arrays of a table, the parser's results, a pass's records) would wait like that.
__global__ __launch_bounds__(256) void k_copy_bytes(unsigned char *__restrict__ dst, const unsigned char *__restrict__ src, size_t bytes) {
    const size_t n16 = bytes / 16;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
        reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    if (blockIdx.x == 0 && threadIdx.x < (bytes & 15)) dst[n16 * 16 + threadIdx.x] = src[n16 * 16 + threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------
// The site masks made on the GPU (mc_ctx_set_reference_motif): what find_and_methylate builds for a motif
// (extract_contexts.py:33-41,:60-81) -- the upper-cased sequence, bit p of the strand mask <=> meth_fwd / meth_rev[p] == 'M' --
// from the raw FASTA bytes and the motif, for every contig at once.  For a motif that cannot overlap itself (no proper prefix
// is also a suffix; the caller checks) str.replace's left-to-right, non-overlapping rule is "every occurrence": position p is
// marked iff an occurrence of the motif starts at p - j for a j whose base is replaced, or the sequence holds an 'M' at p
// already.  Then the site numbering of the per-site reduction: marked sites before every mask word, per (contig, strand).
// ---------------------------------------------------------------------------------------------------
struct MarkMotif { char motif[16], repl[16]; int m; };

__global__ __launch_bounds__(256) void k_mark_upper(const uint8_t *__restrict__ raw, uint8_t *__restrict__ seq, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t ch = raw[i];
        seq[i] = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
    }
}

__device__ __forceinline__ int mark_contig_of_word(const int64_t *__restrict__ word_off, int n_contigs, int64_t gw) {
    int lo = 0, hi = n_contigs - 1;                     // last contig whose first word is <= gw
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (word_off[mid] <= gw) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one thread per mask word and strand pair; cnt[2 * word_off[ci] + st * nw(ci) + w] = marked sites of that word (the order of
// the site numbering: per contig all '+' sites, then all '-' sites)
__global__ __launch_bounds__(256) void k_mark_words(const uint8_t *__restrict__ seq, const int64_t *__restrict__ contig_len,
                                                    const int64_t *__restrict__ seq_off, const int64_t *__restrict__ word_off,
                                                    int n_contigs, int64_t n_words, MarkMotif F, MarkMotif R,
                                                    uint32_t *__restrict__ mf, uint32_t *__restrict__ mr,
                                                    long long *__restrict__ cnt) {
    const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= n_words) return;
    const int ci = mark_contig_of_word(word_off, n_contigs, gw);
    const int64_t w = gw - word_off[ci], L = contig_len[ci];
    const int64_t nw = (ci + 1 < n_contigs ? word_off[ci + 1] : n_words) - word_off[ci];
    const uint8_t *__restrict__ s = seq + seq_off[ci];
    uint32_t bits[2] = {0u, 0u};
    for (int st = 0; st < 2; ++st) {
        const MarkMotif &M = st ? R : F;
        uint32_t b = 0;
        for (int k = 0; k < 32; ++k) {
            const int64_t p = 32 * w + k;
            if (p >= L) break;
            bool marked = s[p] == 'M';
            for (int j = 0; j < M.m && !marked; ++j) {
                if (M.repl[j] != 'M' || M.motif[j] == 'M') continue;           // (not a replaced base of the motif)
                const int64_t q = p - j;
                if (q < 0 || q + M.m > L) continue;
                bool hit = true;
                for (int i = 0; i < M.m && hit; ++i) hit = s[q + i] == (uint8_t)M.motif[i];
                marked = hit;
            }
            b |= marked ? (1u << k) : 0u;
        }
        bits[st] = b;
    }
    mf[gw] = bits[0];
    mr[gw] = bits[1];
    cnt[2 * word_off[ci] + w] = __popc(bits[0]);
    cnt[2 * word_off[ci] + nw + w] = __popc(bits[1]);
}

// off: the exclusive scan of cnt.  rank_f / rank_r[gw] = marked sites of the contig's strand before word gw; site_base[2 ci + st]
__global__ __launch_bounds__(256) void k_mark_ranks(const long long *__restrict__ off, const int64_t *__restrict__ word_off, int n_contigs,
                                                    int64_t n_words, int32_t *__restrict__ rank_f, int32_t *__restrict__ rank_r,
                                                    int64_t *__restrict__ site_base) {
    const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= n_words) return;
    const int ci = mark_contig_of_word(word_off, n_contigs, gw);
    const int64_t w = gw - word_off[ci];
    const int64_t nw = (ci + 1 < n_contigs ? word_off[ci + 1] : n_words) - word_off[ci];
    const long long f0 = off[2 * word_off[ci]], r0 = off[2 * word_off[ci] + nw];
    rank_f[gw] = (int32_t)(off[2 * word_off[ci] + w] - f0);
    rank_r[gw] = (int32_t)(off[2 * word_off[ci] + nw + w] - r0);
    if (w == 0) { site_base[2 * ci] = f0; site_base[2 * ci + 1] = r0; }
}

// ---------------------------------------------------------------------------------------------------
// The site masks of a set of degenerate motifs (mc_ctx_set_reference_iupac; the rule: mc_iupac.h).  k_mark_words compares bytes,
// up to 32 x m x m per lane, and knows one literal motif; here the bases become bit-planes once and a motif is matched 96
// positions at a time: starts = AND over its letters of (the letter set's plane >> i), marks = OR over the called j of
// (starts << j).  kp_scan and k_mark_ranks follow as they do behind k_mark_words.
// ---------------------------------------------------------------------------------------------------
constexpr int IU_PLANES = 5;        // A, C, G, T, and the literal 'M' of the sequence: plane k is planes[k * n_words, (k + 1) * n_words)

// A wave takes 64 bases per step -- two mask words, each half of the wave one (they may lie in two contigs) --, writes the
// upper-cased bytes and, by ballots, the planes on the masks' own word grid (word_off, pad words included).  Past a contig's
// length the planes are zero: nothing matches across a contig end.
__global__ __launch_bounds__(256) void k_ref_planes(const uint8_t *__restrict__ raw, uint8_t *__restrict__ seq,
                                                    const int64_t *__restrict__ contig_len, const int64_t *__restrict__ seq_off,
                                                    const int64_t *__restrict__ word_off, int n_contigs, int64_t n_words,
                                                    uint32_t *__restrict__ planes) {
    const int lane = threadIdx.x & 63, half = lane >> 5, bit = lane & 31;
    const int64_t n_steps = (n_words + 1) / 2;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t step = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; step < n_steps; step += n_waves) {      // (uniform in the wave)
        const int64_t gw = 2 * step + half;
        unsigned ch = 0;
        if (gw < n_words) {
            const int ci = mark_contig_of_word(word_off, n_contigs, gw);
            const int64_t p = 32 * (gw - word_off[ci]) + bit;
            if (p < contig_len[ci]) {
                const int64_t at = seq_off[ci] + p;
                ch = iu_upper(raw[at]);
                seq[at] = (uint8_t)ch;
            }
        }
        const unsigned long long b[IU_PLANES] = {__ballot(ch == 'A'), __ballot(ch == 'C'), __ballot(ch == 'G'), __ballot(ch == 'T'),
                                                 __ballot(ch == 'M')};
        if (bit == 0 && gw < n_words) {
#pragma unroll
            for (int k = 0; k < IU_PLANES; ++k) planes[(int64_t)k * n_words + gw] = (uint32_t)(b[k] >> (32 * half));
        }
    }
}

// one thread per mask word and strand pair, like k_mark_words (and the same cnt layout); S: at most 8 x 2 motifs, by value
__global__ __launch_bounds__(256) void k_mark_iupac(const uint32_t *__restrict__ planes, const int64_t *__restrict__ word_off,
                                                    int n_contigs, int64_t n_words, const mc_iupac_spec S,
                                                    uint32_t *__restrict__ mf, uint32_t *__restrict__ mr,
                                                    long long *__restrict__ cnt) {
    const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= n_words) return;
    const int ci = mark_contig_of_word(word_off, n_contigs, gw);
    const int64_t w = gw - word_off[ci];
    const int64_t nw = (ci + 1 < n_contigs ? word_off[ci + 1] : n_words) - word_off[ci];
    // positions [32 w - 32, 32 w + 64) of the contig: bit 32 of the window is the word's first position
    iu_u128 P[IU_PLANES];
#pragma unroll
    for (int k = 0; k < IU_PLANES; ++k) {
        const uint32_t *__restrict__ pl = planes + (int64_t)k * n_words + word_off[ci];
        const uint32_t lo = w > 0 ? pl[w - 1] : 0u, mid = pl[w], hi = w + 1 < nw ? pl[w + 1] : 0u;
        P[k] = (iu_u128)lo | ((iu_u128)mid << 32) | ((iu_u128)hi << 64);
    }
    iu_u128 f = P[4], r = P[4];                          // a literal 'M' is a mark on both strands
    for (int k = 0; k < S.n_motifs; ++k) {
        f |= iu_window_marks(&S.fwd[k], P[0], P[1], P[2], P[3]);
        r |= iu_window_marks(&S.rev[k], P[0], P[1], P[2], P[3]);
    }
    const uint32_t bf = (uint32_t)(f >> 32), br = (uint32_t)(r >> 32);
    mf[gw] = bf;
    mr[gw] = br;
    cnt[2 * word_off[ci] + w] = __popc(bf);
    cnt[2 * word_off[ci] + nw + w] = __popc(br);
}

struct KpTok { int64_t b; int n; };

__device__ __forceinline__ bool kp_int(const char *__restrict__ t, KpTok k, long long *out) {       // mc_parse.cpp parse_int
    int64_t p = k.b, e = k.b + k.n;
    bool neg = false;
    if (p < e && (t[p] == '+' || t[p] == '-')) { neg = t[p] == '-'; ++p; }
    if (p >= e) return false;
    long long v = 0;
    for (; p < e; ++p) {
        const int d = t[p] - '0';
        if (d < 0 || d > 9) return false;
        v = v * 10 + d;
        if (v > (1ll << 40)) return false;
    }
    *out = neg ? -v : v;
    return true;
}

__device__ __forceinline__ bool kp_e4(const char *__restrict__ t, KpTok k, long long *out) {        // mc_parse.cpp parse_e4_fast
    int64_t p = k.b, e = k.b + k.n;
    bool neg = false;
    if (p < e && (t[p] == '+' || t[p] == '-')) { neg = t[p] == '-'; ++p; }
    long long v = 0;
    int nd = 0, nf = 0;
    for (; p < e && t[p] >= '0' && t[p] <= '9'; ++p) {
        v = v * 10 + (t[p] - '0');
        if (++nd > 9) return false;
    }
    if (p < e && t[p] == '.') {
        ++p;
        for (; p < e && t[p] >= '0' && t[p] <= '9'; ++p) {
            if (++nf > 4) return false;
            v = v * 10 + (t[p] - '0');
        }
    }
    if (p != e || (nd == 0 && nf == 0)) return false;
    for (int i = nf; i < 4; ++i) v *= 10;
    *out = neg ? -v : v;
    return true;
}

__device__ __forceinline__ bool kp_same(const char *__restrict__ t, int64_t a, int64_t b, int n) {
    for (int i = 0; i < n; ++i)
        if (t[a + i] != t[b + i]) return false;
    return true;
}

struct KpParseArgs {
    const char *text;
    int64_t n_bytes;
    const long long *line_start;
    const KpHead *head;
    KpHead *head_w;
    int64_t cap_lines;
    // contigs
    const uint32_t *c_hash;
    const int32_t *c_id;
    const uint32_t *c_off, *c_len;
    const char *c_chars;
    int c_mask;
    // line-indexed output
    int32_t *pos, *idx, *ev, *mu, *contig;
    uint32_t *name_off;
    uint16_t *name_len;
    uint8_t *fl, *status;
};

// One line: t[x - adj] is byte x of the text (t: the staged piece in LDS with adj = its first byte, or the text itself with
// adj = 0; a function of its own so that each call site has ONE address space -- a pointer that is LDS in one branch and
// global in the other becomes a flat pointer, and the flat form of an LDS address must not be offset by hand).
// -> true: the line is a row; *name: its read-name token, in t's coordinates
__device__ __forceinline__ bool kp_parse_line(const KpParseArgs &A, const char *t, const int64_t adj, const int64_t li, const long long n_nl, KpTok *name) {
    const int64_t b = A.line_start[li] - adj;
    const int64_t e = (li + 1 <= n_nl ? A.line_start[li + 1] - 1 : A.n_bytes) - adj;     // the newline, or the end of the text
    KpTok tok[12];
    int nt = 0;
    {
        int64_t s = b;
        while (s < e && nt < 12) {
            while (s < e && kp_is_ws((unsigned char)t[s])) ++s;
            if (s >= e) break;
            const int64_t tb = s;
            while (s < e && !kp_is_ws((unsigned char)t[s])) ++s;
            // (written with a constant index: `tok[nt] = ...` makes the twelve tokens an array in scratch memory, 208 bytes per lane)
            const int tn = (int)min(s - tb, (int64_t)0x7fffffff);
#pragma unroll
            for (int q = 0; q < 12; ++q)
                if (q == nt) { tok[q].b = tb; tok[q].n = tn; }
            ++nt;
        }
    }
    uint8_t st = KP_ST_ROW;
    if (nt < 12) { A.status[li] = KP_ST_SKIP; return false; }             // :149-152
    // contig (:154-160): FNV-1a of the token, probe, compare the bytes
    int32_t contig = -1;
    {
        uint32_t h = 2166136261u;
        for (int i = 0; i < tok[0].n; ++i) h = (h ^ (unsigned char)t[tok[0].b + i]) * 16777619u;
        if (h == 0) h = 1;
        for (int slot = (int)(h & (uint32_t)A.c_mask);; slot = (slot + 1) & A.c_mask) {
            const uint32_t hs = A.c_hash[slot];
            if (hs == 0) break;
            if (hs == h) {
                const int32_t id = A.c_id[slot];
                if ((int)A.c_len[id] == tok[0].n) {
                    bool same = true;
                    for (int i = 0; i < tok[0].n && same; ++i) same = A.c_chars[A.c_off[id] + i] == t[tok[0].b + i];
                    if (same) { contig = id; break; }
                }
            }
        }
    }
    A.name_off[li] = (uint32_t)(tok[0].b + adj);    // (unknown contig: the token is what the message names)
    A.name_len[li] = (uint16_t)min(tok[0].n, 0xFFFF);
    if (contig < 0) { A.status[li] = tok[0].n > 0xFFFF ? KP_ST_HOST : KP_ST_UNKNOWN; if (tok[0].n > 0xFFFF) atomicMin(&A.head_w->first_host_line, (long long)li); return false; }
    long long pos = 0, idx = 0, e4 = 0, m4 = 0;
    if (!kp_int(t, tok[1], &pos) || !kp_int(t, tok[5], &idx)) st = KP_ST_HOST;
    else if (pos < 0 || pos > 0x7fffffffll || idx < -0x7fffffffll || idx > 0x7fffffffll) st = KP_ST_HOST;
    else if (!(kp_e4(t, tok[6], &e4) && kp_e4(t, tok[10], &m4) && e4 > -1000000000ll && e4 < 1000000000ll && m4 > -1000000000ll &&
               m4 < 1000000000ll))
        st = KP_ST_HOST;                            // (float() forms that need strtod: the host parser's slow path)
    if (tok[3].n > 0xFFFF) st = KP_ST_HOST;
    if (st == KP_ST_HOST) {
        A.status[li] = st;
        atomicMin(&A.head_w->first_host_line, (long long)li);
        return false;
    }
    uint8_t fl = 0;
    if (tok[2].n == tok[9].n && kp_same(t, tok[2].b, tok[9].b, tok[2].n)) fl |= MC_F_KMER_EQ;
    if (tok[9].n == 6 && t[tok[9].b] == 'N' && t[tok[9].b + 1] == 'N' && t[tok[9].b + 2] == 'N' && t[tok[9].b + 3] == 'N' &&
        t[tok[9].b + 4] == 'N' && t[tok[9].b + 5] == 'N')
        fl |= MC_F_MODEL_N;
    A.pos[li] = (int32_t)pos;
    A.idx[li] = (int32_t)idx;
    A.ev[li] = (int32_t)e4;
    A.mu[li] = (int32_t)m4;
    A.contig[li] = contig;
    A.name_off[li] = (uint32_t)(tok[3].b + adj);
    A.name_len[li] = (uint16_t)tok[3].n;
    A.fl[li] = fl;
    A.status[li] = KP_ST_ROW;
    *name = tok[3];
    return true;
}

// The 256 lines of a workgroup are one contiguous piece of the text (~30 KB): it is copied into LDS with 16-byte loads and
// the lanes walk their lines there -- a lane reading its line byte by byte from global memory touches a different cache line
// than its 63 neighbours with every load (2.6 ms per 1.25 * 10^6 lines; staged: see DESIGN.md).  A piece that does not fit
// (very long lines) is read in place.
constexpr int KP_STAGE = 48 * 1024;
constexpr uint8_t KP_FL_PREV_KNOWN = 0x40, KP_FL_PREV_SAME = 0x80;     // staging flags of a row (kp_parse -> kp_place): the LINE before it is a row too and carries / does not carry its read name

__global__ __launch_bounds__(256) void kp_parse(KpParseArgs A) {
    extern __shared__ __attribute__((aligned(16))) char s_text[];      // KP_STAGE + 16 bytes
    const long long n_lines = min((long long)A.head->n_lines, (long long)A.cap_lines - 1);
    const int64_t l0 = (int64_t)blockIdx.x * 256;
    if (l0 >= n_lines) return;
    const long long n_nl = A.head->n_newlines;
    const int64_t l1 = min(l0 + 256, (int64_t)n_lines);
    const int64_t g0 = A.line_start[l0], g1 = l1 <= n_nl ? (int64_t)A.line_start[l1] : A.n_bytes;
    const int64_t a0 = g0 & ~(int64_t)15;
    const int64_t li = l0 + threadIdx.x;
    if (g1 - a0 <= KP_STAGE) {                               // (the text buffer is padded: whole 16-byte groups are readable)
        __shared__ int s_nb[256], s_nn[256];                  // the lines' read-name tokens (staged offset, length; -1: the line is no row)
        for (int64_t i = (int64_t)threadIdx.x * 16; i < g1 - a0; i += 256 * 16)
            *reinterpret_cast<uint4 *>(s_text + i) = *reinterpret_cast<const uint4 *>(A.text + a0 + i);
        __syncthreads();
        KpTok name;
        name.b = 0; name.n = -1;
        const bool is_row = li < n_lines && kp_parse_line(A, s_text, a0, li, n_nl, &name);
        s_nb[threadIdx.x] = (int)name.b;
        s_nn[threadIdx.x] = is_row ? name.n : -1;
        __syncthreads();
        // Does the row carry the read name of the LINE before it?  Asked here, where both lines lie in LDS: kp_place, which needs the
        // answer for the row before (nearly always that line), otherwise compares the two names byte by byte in global memory -- 41
        // bytes a row, every load of a lane in another cache line than its neighbours'.  (A workgroup's first line: not known here.)
        if (is_row && threadIdx.x > 0 && s_nn[threadIdx.x - 1] >= 0) {
            const bool same = s_nn[threadIdx.x - 1] == name.n && kp_same(s_text, (int64_t)s_nb[threadIdx.x - 1], name.b, name.n);
            A.fl[li] |= (uint8_t)(KP_FL_PREV_KNOWN | (same ? KP_FL_PREV_SAME : 0));
        }
    } else {
        KpTok name;
        if (li < n_lines) (void)kp_parse_line(A, A.text, 0, li, n_nl, &name);
    }
}

// rows per block of 256 lines
__global__ __launch_bounds__(256) void kp_count_rows(const uint8_t *__restrict__ status, const KpHead *__restrict__ head, int64_t cap_lines,
                                                     long long *__restrict__ blk_cnt) {
    __shared__ int s_w[4];
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const long long n_lines = min((long long)head->n_lines, (long long)cap_lines - 1);
    int c = (li < n_lines && status[li] == KP_ST_ROW) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (long long)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

struct KpPlaceArgs {
    const char *text;
    const KpHead *head;
    KpHead *head_w;
    int64_t cap_lines, cap_rows;
    const long long *blk_off;
    const int32_t *pos, *idx, *ev, *mu, *contig;
    const uint32_t *name_off;
    const uint16_t *name_len;
    const uint8_t *fl, *status;
    // the table slot
    int32_t *t_pos, *t_idx;
    int2 *t_evmu;
    uint8_t *t_flags;
    uint8_t *t_nbits;               // the model-N bit column: one bit per row, made here from the rows' staged flag bytes
    uint16_t *t_xrel;               // the index-relation column: two bits per row, each row's staged index against its predecessor's
    uint16_t *t_prel;               // the position-relation column: two bits per row, its staged position against its predecessor's, and against 0
    int2 *t_unit_pp;                // the unit summaries: the positions of rows 8u and 8u + 7, stored by the threads that place those rows
    KpSeg *segs;
    int cap_segs;
    KpUnknown *unknown;
};

// The model-N bit column (DevTable::nbits) is made here too, a byte per eight rows: the workgroup gathers the bits of its rows in
// LDS, from the row of its first byte on (bit 0 = row base = first row & ~7), and WRITES every byte whose first row is one of
// its own -- the last of these may need the rows of the lines behind the workgroup's, which wave 0 looks up (64 lines at a
// time: status and staged flag byte are all it takes).  A byte that begins with an earlier workgroup's row is that workgroup's.
// So every byte of [0, ceil(n_rows / 8)) is stored exactly once, whole, whatever the slot held before.
// The index-relation column (DevTable::xrel) goes the same way, a 16-bit word per eight rows from two bit planes gathered beside
// the model-N bits ("greater than", "less than" the index of the row before it -- the predecessor every row looks for anyway,
// whatever its name; the table's first row has none and leaves both bits clear), under the same ownership rule.
// The position-relation column (DevTable::prel) likewise, from two more planes: the row's position is less than its predecessor's,
// the row's position is 0.  The unit summaries (DevTable::unit_pp) need no gathering: the thread that places row 8u stores the
// unit's first position, the thread that places row 8u + 7 its last (a table's last, partial unit keeps whatever .y the slot held).
__global__ __launch_bounds__(256) void kp_place(KpPlaceArgs A) {
    __shared__ int s_w[4];
    __shared__ uint32_t s_nbits[10];                // bits of rows base .. base + 319 (7 in front, 256 rows, 7 behind)
    __shared__ uint32_t s_xinc[10], s_xdec[10];     // ... likewise: the row's index is greater / less than its predecessor's
    __shared__ uint32_t s_pdec[10], s_pos0[10];     // ... its position is less than its predecessor's / is 0
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t li = (int64_t)blockIdx.x * 256 + tid;
    const long long n_lines = min((long long)A.head->n_lines, (long long)A.cap_lines - 1);
    const uint8_t st = li < n_lines ? A.status[li] : (uint8_t)KP_ST_SKIP;
    const bool is_row = st == KP_ST_ROW;
    const unsigned long long bal = __ballot(is_row);
    if (lane == 0) s_w[wave] = __popcll(bal);
    if (tid < 10) s_nbits[tid] = s_xinc[tid] = s_xdec[tid] = s_pdec[tid] = s_pos0[tid] = 0u;
    __syncthreads();
    // the row before a row: the line before it, unless that one is no row (-1: the table's first row)
    auto row_before = [&](int64_t l) {
        int64_t q = l - 1;
        while (q >= 0 && A.status[q] != KP_ST_ROW) --q;
        return q;
    };
    // (bit `at` of the planes from a row's index and position and its predecessor's)
    auto note_rel = [&](int at, int64_t l, int64_t q) {
        const int32_t pi = A.pos[l];
        if (pi == 0) atomicOr(&s_pos0[at >> 5], 1u << (at & 31));
        if (q < 0) return;
        const int32_t xi = A.idx[l], xq = A.idx[q];
        if (xi > xq) atomicOr(&s_xinc[at >> 5], 1u << (at & 31));
        if (xi < xq) atomicOr(&s_xdec[at >> 5], 1u << (at & 31));
        if (pi < A.pos[q]) atomicOr(&s_pdec[at >> 5], 1u << (at & 31));
    };
    const int64_t pl = is_row ? row_before(li) : -1;
    const long long row0 = A.blk_off[blockIdx.x];
    long long row = row0 + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) row += s_w[w];
    {
        const long long row_end = row0 + s_w[0] + s_w[1] + s_w[2] + s_w[3], base = row0 & ~7ll;
        if (is_row && (A.fl[li] & MC_F_MODEL_N)) atomicOr(&s_nbits[(int)(row - base) >> 5], 1u << ((int)(row - base) & 31));
        if (is_row) note_rel((int)(row - base), li, pl);
        // (the rows behind the workgroup's that share its last byte -- only if that byte begins with one of its rows)
        int need = (int)((8 - (row_end & 7)) & 7);
        if (wave == 0 && row_end > row0 && ((row_end - 1) & ~7ll) >= row0 && need > 0) {
            long long r = row_end;
            for (int64_t l0 = (int64_t)blockIdx.x * 256 + 256; need > 0 && l0 < n_lines; l0 += 64) {       // (wave-uniform)
                const int64_t l = l0 + lane;
                const bool rw = l < n_lines && A.status[l] == KP_ST_ROW;
                const unsigned long long rb = __ballot(rw);
                const int nth = __popcll(rb & ((1ull << lane) - 1ull));
                if (rw && nth < need && (A.fl[l] & MC_F_MODEL_N)) atomicOr(&s_nbits[(int)(r + nth - base) >> 5], 1u << ((int)(r + nth - base) & 31));
                // (its predecessor -- the row lane before it in the ballot, for the first one the workgroup's last row -- found as
                // every row finds its own: at most seven lanes walk back over the lines that are no rows)
                if (rw && nth < need) note_rel((int)(r + nth - base), l, row_before(l));
                const int got = min(__popcll(rb), need);
                r += got;
                need -= got;
            }
        }
        __syncthreads();
        // bytes [b0, b1): those whose first row is in [row0, row_end) (and inside the slot)
        const long long b0 = (row0 + 7) >> 3, b1 = min((row_end + 7) >> 3, (long long)((A.cap_rows + 7) >> 3));
        if (b0 + tid < b1) {
            const int off = (int)(b0 + tid - (base >> 3));
            A.t_nbits[b0 + tid] = (uint8_t)(s_nbits[off >> 2] >> (8 * (off & 3)));
            A.t_xrel[b0 + tid] = (uint16_t)(((s_xinc[off >> 2] >> (8 * (off & 3))) & 0xFFu) | (((s_xdec[off >> 2] >> (8 * (off & 3))) & 0xFFu) << 8));
            A.t_prel[b0 + tid] = (uint16_t)(((s_pdec[off >> 2] >> (8 * (off & 3))) & 0xFFu) | (((s_pos0[off >> 2] >> (8 * (off & 3))) & 0xFFu) << 8));
        }
    }
    if (st == KP_ST_UNKNOWN) {                          // :156-160: the line is skipped, the message names the contig
        const int k = atomicAdd(&A.head_w->n_unknown, 1);
        if (k < KP_MAX_UNKNOWN) { KpUnknown u; u.line = li; u.off = A.name_off[li]; u.len = A.name_len[li]; u.pad = 0; A.unknown[k] = u; }
        else atomicOr(&A.head_w->overflow, 4);
    }
    if (!is_row) return;
    if (row >= A.cap_rows) { atomicOr(&A.head_w->overflow, 1); return; }
    const uint32_t no = A.name_off[li];
    const int nl = A.name_len[li];
    bool new_name = true, new_seg = true;
    const uint8_t fl_staged = A.fl[li];
    if (pl >= 0) {
        if (pl == li - 1 && (fl_staged & KP_FL_PREV_KNOWN)) new_name = !(fl_staged & KP_FL_PREV_SAME);        // (kp_parse compared them in LDS)
        else new_name = A.name_len[pl] != nl || !kp_same(A.text, (int64_t)A.name_off[pl], (int64_t)no, nl);
        new_seg = new_name || A.contig[pl] != A.contig[li];
    }
    uint8_t fl = fl_staged & (uint8_t)~(KP_FL_PREV_KNOWN | KP_FL_PREV_SAME);
    if (new_name) fl |= MC_F_NAME_START;
    if (new_seg) {
        fl |= MC_F_SEG_START;
        const int k = atomicAdd(&A.head_w->n_seg, 1);
        if (k < A.cap_segs) { KpSeg s; s.row = row; s.name_off = no; s.name_len = nl; s.contig = A.contig[li]; s.name_start = new_name ? 1 : 0; s.pad = 0; A.segs[k] = s; }
        else atomicOr(&A.head_w->overflow, 2);
    }
    const int32_t p_staged = A.pos[li];
    A.t_pos[row] = p_staged;
    if ((row & 7) == 0) A.t_unit_pp[row >> 3].x = p_staged;
    if ((row & 7) == 7) A.t_unit_pp[row >> 3].y = p_staged;
    A.t_idx[row] = A.idx[li];
    A.t_evmu[row] = make_int2(A.ev[li], A.mu[li]);
    A.t_flags[row] = fl;
}

#endif  // MC_LINES_ONLY

}  // namespace
