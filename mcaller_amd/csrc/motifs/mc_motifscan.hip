// mc_motifscan.hip -- methylated motifs found de novo from called sites on the GPU: for every shape of X and '.', every X of it as
// the called letter and every assignment of A, C, G, T to the X, how many candidates of the reference stand in such a window
// (nGenome), how many of them are covered and how many methylated; the rows that are mostly methylated, less those a shorter
// selected row explains, in order, as text -- what find_motifs.find_motifs builds in NumPy (C ABI: mc_motif_report,
// mc_motif_report_last_stats, mc_motif_report_release; Python: Device.motif_report, find_motifs.find_motifs_device).  The unit
// stands in csrc/motifs/, beside csrc/bed/, csrc/train/, csrc/merge/, csrc/fastq/ and csrc/compare/: no pass runs its kernels.
//
// The result is the host statement's bytes or a decline (status 1, mc_last_error; the stats say which file and line):
//   MC_MOTIF_DECLINE_HIGH_BYTE   a byte >= 0x80                  MC_MOTIF_DECLINE_CONTROL    a control byte other than tab and newline
//   MC_MOTIF_DECLINE_LONG_LINE   a line over 65535 bytes         MC_MOTIF_DECLINE_FIELDS     fewer than 6 tab-separated fields
//   MC_MOTIF_DECLINE_FIELD       an empty chrom, a start that is not plain digits, a strand other than + / -
//   MC_MOTIF_DECLINE_CHROM       a chrom that is no contig       MC_MOTIF_DECLINE_RANGE      a start outside its contig
//   MC_MOTIF_DECLINE_TABLE       the contig table is full (MCALLER_MOTIF_TABLE_SLOTS forces one)
//   MC_MOTIF_DECLINE_MEMORY      it does not fit device memory   MC_MOTIF_DECLINE_REFERENCE  2^31 bases or more (counters are 32-bit)
//   MC_MOTIF_DECLINE_PRINT       a fraction mc_rowtext.h does not print      MC_MOTIF_DECLINE_ROWS   2^31 - 2 lines or more
// Of several offending lines the first is named, the bed's before the control's; of several reasons on it the smallest: line_flag
// (mc_textdev.h) over the lines of both texts, which stand behind one another in one device buffer as in compare/mc_bedcompare.hip.
//
// The genome on the device.  Contig c begins at base index gstart[c], a multiple of 64 that leaves at least 32 bases of padding
// behind the contig before it; 64 bases of padding stand in front of the first contig and two words behind the last.  Three
// bit-planes, 64 bases a word: the two bits of a base's code (A 0, C 1, G 2, T 3) and `valid` (the base is one of ACGT; padding is
// not).  A window of up to 24 bases whose first and last letter are valid lies inside ONE contig, because the padding is wider
// than a window: "inside the contig" and "every letter under an X is ACGT" are one test against `valid`.  Four more planes per
// strand: candidate (the base on that strand is --base), methylated and control (the sites the two files list, atomicOr: the
// order of the lines does not matter and a site listed twice counts once).
//   km_pack      a lane per base index: the contig by binary search, the letter, five wave ballots -> a word of each plane
//   km_contigs   a lane per contig: its id's KeyHash, kt_claim into the contig table (ids are contig numbers)
//   kp_count / kp_scan / kp_starts   line starts of the two texts (mc_lines.h, launched by mc_textfeed.h)
//   km_parse     a lane per line: ByteClass, the first six tabs, the start in integers, kt_find of the chrom, the site's bit
//   km_figures   popcounts of the planes: candidates, listed sites, control sites, listed sites off base
//   km_count     THE HOT PATH, one launch per table (shape, j), a workgroup per stretch of the genome (MCALLER_MOTIF_STRETCH bases,
//                a multiple of 64; 65536 unless the genome is shorter).  A lane takes a base index; where it is a candidate (of
//                either strand: no base is both) it funnels the 47 bases around it out of two words of each plane into three
//                registers, tests the table's X mask against `valid`, and gathers the letters under the X -- on '-' from the
//                mirrored offsets, complemented (both code bits flipped).  The called letter is always --base, so a table has
//                4^(k-1) used entries and the key leaves that letter out: 64 KB of 32-bit counters for 8 X.
//                  LDS placement     the table is a histogram in dynamic LDS (ds_add), zeroed before and flushed behind the
//                                    stretch with one global integer atomicAdd per NON-ZERO entry, consecutive lanes on
//                                    consecutive entries
//                  global placement  a table with more used entries than a stretch has candidate slots (2 x stretch): zeroing
//                                    and flushing would issue more LDS and global traffic than the counts themselves, so the few
//                                    counts go straight to global memory.  At the default stretch every table is in LDS.
//                nCovered and nMethylated, far rarer, go straight to global memory; without a control nCovered IS nGenome
//   km_select    a lane per entry: nMethylated >= min_sites and one IEEE fp64 division against min_fraction
//   km_keep      a selected entry reads, for every (shape', j') that embeds in its own (the host lists them with the letter each
//                parent letter comes from), the parent's selected flag at the parent's key: set -> dropped.  Counts the survivors
//   km_gather    the survivors' (entry, nGenome, nCovered, nMethylated) into a list, slots by atomicAdd: the host sorts them by
//                the integer keys of the definition (they are few) and writes SPEC and the numbers with mc_rowtext.h
//   --iupac      behind km_count, in place of km_select / km_keep / km_gather: mc_motifiupac.inc (C ABI: mc_motif_report's iupac,
//                mc_motif_report_iupac_last_stats)
//   --iterative  behind km_count, round after round: the selection above (ms_rows, or mi_rows of mc_motifiupac.inc) gives the ordered
//                rows in structured form, the first is printed, km_explain takes the candidates it explains out of the candidate
//                planes and km_uncount out of every table (ms_key: the one statement of a window's validity and key, shared with
//                km_count), and the selection runs again: mc_motifiter.inc (C ABI: mc_motif_report's max_motifs, _iter_last_stats,
//                _iter_left: the methylated candidates no row explains, as two planes in pinned memory)
//   motif_profile  another question over the same planes -- given motifs counted per contig or window, and every bin's nearest bins:
//                mc_motifprofile.inc (C ABI: mc_motif_profile, _last_stats, _release); km_pack, km_contigs, km_parse and km_figures
//                run there as they are, nothing of it runs in a mc_motif_report call
// No floating-point atomic anywhere; the counts are exact integers whatever the order of arrival.
#include "../mc_textfeed.h"
#include "../mc_rowtext.h"
#include "../mc_iupac.h"

#include <cstdio>
#include <cstring>
#include <string>

namespace {

constexpr unsigned long long MS_NO_DECLINE = ~0ull;
constexpr int MS_REACH = MC_MOTIF_MAX_WIDTH - 1;       // bases a window reaches to either side of its called letter
constexpr int64_t MS_STRETCH = 65536;

struct MsHead {                              // device-side result block (copied to the host as it is)
    KpHead kp;
    unsigned long long decline;              // min over the offending lines of line << 8 | reason (~0: none)
    long long n_lines1;                      // lines that start before the control's text
    unsigned long long n_candidates, n_sites, n_control, n_off_base, n_selected, n_rows, cursor;
    int table_full, pad;
    unsigned long long n_list, n_left;       // --iterative: candidates the round's row explains; methylated candidates left
};

struct MsTable {                             // a (shape, j)
    uint64_t mask[2];                        // the X of the shape as bits of the 47-base neighbourhood, '+' and '-'
    uint32_t off, entries;                   // its counters: [off, off + entries), entries = 4^(k - 1)
    int32_t shape, k, j, o, W;
    int32_t parent_lo, parent_hi;            // its parents in MsParent[]
    uint64_t idx[2];                         // byte i: where the letter under X i stands in the neighbourhood, '+' and '-'
    int8_t x[8];
    uint64_t lat;                            // --iupac: its purity lattice begins here (mc_motifiupac.inc)
};

struct MsParent {
    int32_t table;
    int8_t from[8];                          // the parent's letter i is the child's letter from[i]
};

struct MsRow { uint32_t entry, nG, nC, nM; };

struct MsArgs {
    // the genome
    const uint8_t *seq;
    const int64_t *contig_len, *seq_off, *gstart;
    int32_t n_contigs, base_code;
    int64_t n_words;                         // words of a plane
    uint64_t *code0, *code1, *valid, *cand[2];
    unsigned long long *meth[2], *ctl[2];
    // the contig table
    const char *ids;
    const int64_t *id_off;
    unsigned long long *table;
    uint64_t table_mask, hash_mask;
    // the texts
    const char *text;
    int64_t n_bytes, off2, n_nl;
    const long long *line_start;
    MsHead *head;
    // the tables
    const MsTable *tables;
    const MsParent *parents;
    int32_t n_tables, has_control, keep_all, pad;
    int64_t stretch, G, n_entries;
    unsigned int *nG, *nC, *nM;
    uint8_t *selected, *keep;
    long long min_sites;
    double min_fraction;
    MsRow *rows;
    int64_t cap_rows;
    // --iterative (mc_motifiter.inc)
    long long *list;                         // the candidates a round's row explains: base index << 1 | strand
    int64_t cap_list;
    uint64_t *left;                          // meth & cand of '+', then of '-'
};

__device__ __forceinline__ int ms_code(unsigned c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

__global__ __launch_bounds__(256) void km_pack(MsArgs A) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (the grid covers whole words: n_words * 64 lanes)
    int lo = 0, hi = A.n_contigs;                                    // the last contig that begins at or before g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.gstart[mid] <= g) lo = mid; else hi = mid;
    }
    int code = 4;
    if (A.n_contigs > 0 && g >= A.gstart[lo] && g - A.gstart[lo] < A.contig_len[lo]) code = ms_code(A.seq[A.seq_off[lo] + (g - A.gstart[lo])]);
    const bool ok = code < 4;
    const uint64_t b0 = __ballot(ok && (code & 1)), b1 = __ballot(ok && (code & 2)), v = __ballot(ok);
    const uint64_t cp = __ballot(code == A.base_code), cm = __ballot(ok && code == 3 - A.base_code);
    const int64_t w = g >> 6;
    if ((threadIdx.x & 63) == 0 && w < A.n_words) {
        A.code0[w] = b0; A.code1[w] = b1; A.valid[w] = v; A.cand[0][w] = cp; A.cand[1][w] = cm;
    }
}

__device__ __forceinline__ bool ms_same_id(const MsArgs &A, const char *p, int n, int64_t r) {
    const int64_t b = A.id_off[r];
    return A.id_off[r + 1] - b == n && same_bytes(p, A.ids + b, n);
}

__global__ __launch_bounds__(256) void km_contigs(MsArgs A) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= A.n_contigs) return;
    const char *p = A.ids + A.id_off[c];
    const int n = (int)(A.id_off[c + 1] - A.id_off[c]);
    KeyHash H;
    H.span(p, n);
    const uint64_t h = H.done(A.hash_mask);
    const KtHit hit = kt_claim(A.table, A.table_mask, h, c, [&](int64_t r) { return ms_same_id(A, p, n, r); });
    if (hit.slot < 0) A.head->table_full = 1;
}

__global__ __launch_bounds__(256) void km_parse(MsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_lines = A.head->kp.n_lines;
    if (li >= n_lines) return;
    const int64_t b = A.line_start[li];
    const int64_t e = li < A.n_nl ? (int64_t)A.line_start[li + 1] - 1 : A.n_bytes;
    if (b < A.off2 && (li + 1 >= n_lines || (int64_t)A.line_start[li + 1] >= A.off2)) A.head->n_lines1 = li + 1;      // the bed's last line alone
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_LONG_LINE); return; }
    const char *t = A.text + b;
    const int len = (int)(e - b);
    ByteClass bad;
    int tab[6] = {0, 0, 0, 0, 0, 0}, nt = 0;
    for (int i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)t[i];
        bad.see(c);
        if (c == '\t') {
#pragma unroll
            for (int k = 0; k < 6; ++k) tab[k] = nt == k ? i : tab[k];
            ++nt;
        }
    }
    if (bad.hi) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_HIGH_BYTE); return; }
    if (bad.ctrl) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_CONTROL); return; }
    if (nt < 5) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_FIELDS); return; }
    // chrom [0, t0), start (t0, t1), strand (t4, t5) or (t4, len) on a line of six fields
    const int strand_end = nt >= 6 ? tab[5] : len;
    const unsigned sc = strand_end - tab[4] == 2 ? (unsigned char)t[tab[4] + 1] : 0u;
    bool plain = tab[0] > 0 && tab[1] - tab[0] > 1 && (sc == '+' || sc == '-');
    long long start = 0;
    for (int i = tab[0] + 1; i < tab[1]; ++i) {
        const unsigned d = (unsigned)(unsigned char)t[i] - '0';
        plain = plain && d < 10u;
        start = start * 10 + (long long)(d < 10u ? d : 0u);
        start = start > (1ll << 40) ? (1ll << 40) : start;             // (beyond every contig: the digits behind change nothing)
    }
    if (!plain) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_FIELD); return; }
    KeyHash H;
    H.span(t, tab[0]);
    const uint64_t h = H.done(A.hash_mask);
    const KtHit hit = kt_find(A.table, A.table_mask, h, [&](int64_t r) { return ms_same_id(A, t, tab[0], r); });
    if (hit.id < 0 || hit.id >= A.n_contigs) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_CHROM); return; }
    if (start >= A.contig_len[hit.id]) { line_flag(&A.head->decline, li, MC_MOTIF_DECLINE_RANGE); return; }
    const int64_t g = A.gstart[hit.id] + start;
    unsigned long long *plane = (b < A.off2 ? A.meth : A.ctl)[sc == '-' ? 1 : 0];
    atomicOr(&plane[g >> 6], 1ull << (g & 63));
}

__global__ __launch_bounds__(256) void km_figures(MsArgs A) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long n_cand = 0, n_sites = 0, n_ctl = 0, n_off = 0;
    if (w < A.n_words)
        for (int s = 0; s < 2; ++s) {
            const uint64_t c = A.cand[s][w], m = A.meth[s][w], k = A.ctl[s][w];
            n_cand += __popcll(c); n_sites += __popcll(m); n_ctl += __popcll(k); n_off += __popcll((m | k) & ~c);
        }
    for (int o = 32; o > 0; o >>= 1) {
        n_cand += __shfl_xor(n_cand, o); n_sites += __shfl_xor(n_sites, o); n_ctl += __shfl_xor(n_ctl, o); n_off += __shfl_xor(n_off, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_cand) atomicAdd(&A.head->n_candidates, n_cand);
        if (n_sites) atomicAdd(&A.head->n_sites, n_sites);
        if (n_ctl) atomicAdd(&A.head->n_control, n_ctl);
        if (n_off) atomicAdd(&A.head->n_off_base, n_off);
    }
}

// bits [g0, g0 + 64) of a plane (g0 >= 0; the planes have two words of padding behind the genome)
__device__ __forceinline__ uint64_t ms_funnel(const uint64_t *plane, int64_t g0) {
    const int64_t w = g0 >> 6;
    const int s = (int)(g0 & 63);
    const uint64_t lo = plane[w], hi = plane[w + 1];
    return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// the window of table T around the candidate at base index g of strand s -> false: it does not count; else its key.  Bit i of the
// neighbourhood is base g - MS_REACH + i (g >= 64 > MS_REACH: the first contig begins at 64); on '-' the letters stand at the
// mirrored offsets and are complemented (both code bits flipped).  km_count adds with it and km_uncount takes away
__device__ __forceinline__ bool ms_key(const MsArgs &A, const MsTable &T, int64_t g, int s, uint32_t *key_out) {
    const uint64_t nv = ms_funnel(A.valid, g - MS_REACH);
    const uint64_t mask = T.mask[s], idx = T.idx[s];
    if ((nv & mask) != mask) return false;
    const uint64_t n0 = ms_funnel(A.code0, g - MS_REACH), n1 = ms_funnel(A.code1, g - MS_REACH);
    const uint64_t flip = s ? ~0ull : 0ull;                          // '-': the complement, 3 - code
    const uint64_t c0 = n0 ^ flip, c1 = n1 ^ flip;
    const int k = T.k, j = T.j;
    uint32_t key = 0;
    for (int i = 0; i < k; ++i) {
        if (i == j) continue;
        const int at = (int)((idx >> (8 * i)) & 63ull);
        key = (key << 2) | (uint32_t)((c0 >> at) & 1ull) | ((uint32_t)((c1 >> at) & 1ull) << 1);
    }
    *key_out = key;
    return key < T.entries;                                          // (always: k - 1 letters of two bits)
}

template <bool IN_LDS>
__global__ __launch_bounds__(256) void km_count(MsArgs A, int ti) {
    extern __shared__ unsigned int s_hist[];
    const MsTable &T = A.tables[ti];
    const int64_t g_lo = (int64_t)blockIdx.x * A.stretch, g_hi = min(g_lo + A.stretch, A.G);
    if (IN_LDS) {
        for (uint32_t i = threadIdx.x; i < T.entries; i += 256) s_hist[i] = 0u;
        __syncthreads();
    }
    for (int64_t g = g_lo + threadIdx.x; g < g_hi; g += 256) {
        const int64_t w = g >> 6;
        const int bit = (int)(g & 63);
        const bool plus = (A.cand[0][w] >> bit) & 1ull, minus = (A.cand[1][w] >> bit) & 1ull;
        if (!plus && !minus) continue;                               // (no base is a candidate of both strands)
        const int s = minus ? 1 : 0;
        uint32_t key;
        if (!ms_key(A, T, g, s, &key)) continue;
        if (IN_LDS) atomicAdd(&s_hist[key], 1u);
        else atomicAdd(&A.nG[T.off + key], 1u);
        const bool is_meth = (A.meth[s][w] >> bit) & 1ull;
        if (is_meth) atomicAdd(&A.nM[T.off + key], 1u);
        if (A.has_control && (is_meth || ((A.ctl[s][w] >> bit) & 1ull))) atomicAdd(&A.nC[T.off + key], 1u);
    }
    if (IN_LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < T.entries; i += 256) {
            const unsigned int v = s_hist[i];
            if (v) atomicAdd(&A.nG[T.off + i], v);
        }
    }
}

// the table of entry e: the last one that begins at or before it
__device__ __forceinline__ int ms_table_of(const MsArgs &A, uint32_t e) {
    int lo = 0, hi = A.n_tables;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.tables[mid].off <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// --iterative, rounds 2 on: the counters of the three kernels below begin at 0 again
__global__ void km_again(MsArgs A) {
    if (threadIdx.x == 0) { A.head->n_selected = 0; A.head->n_rows = 0; A.head->cursor = 0; }
}

__global__ __launch_bounds__(256) void km_select(MsArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n_entries) return;
    const unsigned int nM = A.nM[e], nC = A.has_control ? A.nC[e] : A.nG[e];
    const bool sel = (long long)nM >= A.min_sites && (double)nM / (double)nC >= A.min_fraction;      // (0 / 0 is nan: not selected)
    A.selected[e] = sel ? 1 : 0;
    const uint64_t any = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&A.head->n_selected, (unsigned long long)__popcll(any));
}

__global__ __launch_bounds__(256) void km_keep(MsArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (e < A.n_entries && A.selected[e]) {
        keep = true;
        if (!A.keep_all) {
            const MsTable &T = A.tables[ms_table_of(A, (uint32_t)e)];
            const uint32_t key = (uint32_t)e - T.off;
            // the child's letters: the key's digits, the called letter put back
            int letter[8];
            for (int i = T.k - 1, d = 0; i >= 0; --i) {
                if (i == T.j) { letter[i] = A.base_code; continue; }
                letter[i] = (int)((key >> (2 * d)) & 3u);
                ++d;
            }
            for (int p = T.parent_lo; p < T.parent_hi && keep; ++p) {
                const MsParent &P = A.parents[p];
                const MsTable &U = A.tables[P.table];
                uint32_t pk = 0;
                for (int i = 0; i < U.k; ++i)
                    if (i != U.j) pk = (pk << 2) | (uint32_t)letter[P.from[i]];
                if (pk < U.entries && A.selected[U.off + pk]) keep = false;
            }
        }
    }
    if (e < A.n_entries) A.keep[e] = keep ? 1 : 0;
    const uint64_t any = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&A.head->n_rows, (unsigned long long)__popcll(any));
}

__global__ __launch_bounds__(256) void km_gather(MsArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n_entries || !A.keep[e]) return;
    const unsigned long long at = atomicAdd(&A.head->cursor, 1ull);
    if ((int64_t)at >= A.cap_rows) return;                             // (cannot be: km_keep counted these entries)
    A.rows[at] = MsRow{(uint32_t)e, A.nG[e], A.has_control ? A.nC[e] : A.nG[e], A.nM[e]};
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

const char *ms_reason_text(int reason) {
    switch (reason) {
        case MC_MOTIF_DECLINE_HIGH_BYTE: return "a byte >= 0x80";
        case MC_MOTIF_DECLINE_CONTROL: return "a control byte other than tab and newline";
        case MC_MOTIF_DECLINE_LONG_LINE: return "a line longer than 65535 bytes";
        case MC_MOTIF_DECLINE_FIELDS: return "a line with fewer than 6 tab-separated fields";
        case MC_MOTIF_DECLINE_FIELD: return "an empty chrom, a start that is not plain digits or a strand other than + and -";
        case MC_MOTIF_DECLINE_CHROM: return "a chrom that is no contig of the reference";
        case MC_MOTIF_DECLINE_RANGE: return "a start outside its contig";
        case MC_MOTIF_DECLINE_TABLE: return "the contig table is full";
        case MC_MOTIF_DECLINE_MEMORY: return "the reference, the texts and the tables do not fit into free device memory";
        case MC_MOTIF_DECLINE_REFERENCE: return "a reference of 2^31 bases or more";
        case MC_MOTIF_DECLINE_PRINT: return "a fraction the device's row writer does not print";
        case MC_MOTIF_DECLINE_ROWS: return "2^31 - 2 lines or more";
    }
    return "unknown";
}

// file: 1 (the bed), 2 (the control) or 0; line: in that file, -1: none
int ms_decline(mc_ctx *c, int32_t *status, int reason, int file, long long line) {
    static const char *const nouns[2] = {"bed", "control"};
    return decline_in_file(c->motif.stats, status, "motif finder", ms_reason_text(reason), nouns, reason, file, line);
}

int ms_decline_head(mc_ctx *c, int32_t *status, const MsHead &h) {
    const long long line = decline_line(h.decline);
    const bool first = line < h.n_lines1;
    return ms_decline(c, status, decline_reason(h.decline), first ? 1 : 2, first ? line : line - h.n_lines1);
}

// device_fits, or (tests) as if MCALLER_MOTIF_DEVICE_BYTES were all the device had free
bool ms_fits(size_t bytes) { return fits("MCALLER_MOTIF_DEVICE_BYTES", bytes); }

// the tables of the shapes and, for every table, the tables that embed in it -> false: the params are not what the header allows
bool ms_tables(const mc_motif_params &P, std::vector<MsTable> &tables, std::vector<MsParent> &parents) {
    if (P.n_shapes < 1 || P.n_shapes > MC_MOTIF_MAX_SHAPES) return false;
    uint32_t off = 0;
    for (int s = 0; s < P.n_shapes; ++s) {
        const char *shape = P.shapes[s];
        const int W = (int)strnlen(shape, sizeof P.shapes[s]);
        if (W < 2 || W > MC_MOTIF_MAX_WIDTH || shape[0] != 'X' || shape[W - 1] != 'X') return false;
        int x[8], k = 0;
        for (int i = 0; i < W; ++i) {
            if (shape[i] != 'X' && shape[i] != '.') return false;
            if (shape[i] == 'X') { if (k == 8) return false; x[k++] = i; }
        }
        for (int j = 0; j < k; ++j) {
            MsTable T = {};
            T.shape = s; T.k = k; T.j = j; T.o = x[j]; T.W = W;
            T.off = off; T.entries = 1u << (2 * (k - 1));
            off += T.entries;
            for (int i = 0; i < k; ++i) {
                T.x[i] = (int8_t)x[i];
                const int at[2] = {MS_REACH - T.o + x[i], MS_REACH + T.o - x[i]};
                for (int s2 = 0; s2 < 2; ++s2) {
                    T.idx[s2] |= (uint64_t)at[s2] << (8 * i);
                    T.mask[s2] |= 1ull << at[s2];
                }
            }
            tables.push_back(T);
        }
    }
    for (MsTable &T : tables) {
        T.parent_lo = (int32_t)parents.size();
        for (size_t u = 0; u < tables.size(); ++u) {
            const MsTable &U = tables[u];
            if (U.k >= T.k) continue;                                  // a strict subset has fewer letters
            MsParent Pn = {};
            Pn.table = (int32_t)u;
            bool all = true;
            for (int i = 0; i < U.k && all; ++i) {
                int found = -1;
                for (int q = 0; q < T.k; ++q)
                    if (T.x[q] - T.o == U.x[i] - U.o) found = q;
                all = found >= 0;
                Pn.from[i] = (int8_t)(found < 0 ? 0 : found);
            }
            if (all) parents.push_back(Pn);
        }
        T.parent_hi = (int32_t)parents.size();
    }
    return true;
}

struct MsText {                              // the rows' bytes, built on the host
    std::string s;
    void put(char c) { s.push_back(c); }
};

// behind a row's SPEC: ':', the 1-based index of the called letter, the three counts and the fraction -> false: mc_rowtext.h does
// not print the fraction
bool ms_put_numbers(MsText &text, int o, uint32_t nG, uint32_t nC, uint32_t nM) {
    text.put(':');
    rt_put_uint(text, (uint32_t)(o + 1)); text.put('\t');
    rt_put_uint(text, nG); text.put('\t');
    rt_put_uint(text, nC); text.put('\t');
    rt_put_uint(text, nM); text.put('\t');
    if (!rt_put_repr(text, (double)nM / (double)nC)) return false;
    text.put('\n');
    return true;
}

// the rows' bytes into the context's pinned block, handed out (built on the host: a memcpy, no fetch_out)
int ms_hand_out(mc_ctx *c, const MsText &text, std::chrono::steady_clock::time_point t_d2h, const char **out, int64_t *n_out) {
    mc_motif_stats &S = c->motif.stats;
    if (int rc = c->motif.out.need(text.s.size())) return rc;
    memcpy(c->motif.out.get<char>(), text.s.data(), text.s.size());
    S.ms_d2h = ms_since(t_d2h);
    S.n_out_bytes = (int64_t)text.s.size();
    *out = c->motif.out.get<char>();
    *n_out = (int64_t)text.s.size();
    return 0;
}

// The tables are counted -> the rows of the definition in its order, in structured form.  again (--iterative, rounds 2 on): the
// head's counters are zeroed first and the stats keep round 1's figures
int ms_rows(mc_ctx *c, Pool &pool, MsArgs &A, MsHead *d_head, bool again, std::vector<MsRow> &rows, std::chrono::steady_clock::time_point *t_d2h,
            int32_t *status) {
    mc_motif_stats &S = c->motif.stats;
    hipStream_t st = c->stream;
    MsHead h = {};
    rows.clear();
    *t_d2h = std::chrono::steady_clock::now();
    if (again) hipLaunchKernelGGL(km_again, dim3(1), dim3(64), 0, st, A);
    hipLaunchKernelGGL(km_select, dim3(blocks(A.n_entries)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(km_keep, dim3(blocks(A.n_entries)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    const int64_t NR = (int64_t)h.n_rows;
    if (!again) { S.n_selected = (int64_t)h.n_selected; S.n_rows = NR; }
    if (NR == 0) return 0;
    if (NR > A.cap_rows) {
        if (!ms_fits((size_t)NR * sizeof(MsRow) + ((size_t)1 << 20))) return ms_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        if (pool.get(&A.rows, (size_t)NR)) return -10;
        A.cap_rows = NR;
    }
    hipLaunchKernelGGL(km_gather, dim3(blocks(A.n_entries)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    *t_d2h = std::chrono::steady_clock::now();
    rows.resize((size_t)NR);
    HIP_TRY(hipMemcpyAsync(rows.data(), A.rows, (size_t)NR * sizeof(MsRow), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the order of the definition: nMethylated and the fraction descending, then the entry (tables stand in shape and j order,
    // a table's keys in the letters' order)
    std::sort(rows.begin(), rows.end(), [](const MsRow &a, const MsRow &b) {
        if (a.nM != b.nM) return a.nM > b.nM;
        const double fa = (double)a.nM / (double)a.nC, fb = (double)b.nM / (double)b.nC;
        if (fa != fb) return fa > fb;
        return a.entry < b.entry;
    });
    return 0;
}

inline size_t ms_table_of_entry(const std::vector<MsTable> &tables, uint32_t entry) {
    size_t ti = 0;
    while (ti + 1 < tables.size() && tables[ti + 1].off <= entry) ++ti;
    return ti;
}

// a row's line -> false: mc_rowtext.h does not print the fraction
bool ms_line(MsText &text, const mc_motif_params &P, const std::vector<MsTable> &tables, const MsRow &r) {
    const MsTable &T = tables[ms_table_of_entry(tables, r.entry)];
    const uint32_t key = r.entry - T.off;
    const char *shape = P.shapes[T.shape];
    for (int i = 0, x = 0, d = T.k - 2; i < T.W; ++i) {
        if (shape[i] != 'X') { text.put('N'); continue; }
        if (x == T.j) text.put((char)P.base);
        else { text.put("ACGT"[(key >> (2 * d)) & 3u]); --d; }
        ++x;
    }
    return ms_put_numbers(text, T.o, r.nG, r.nC, r.nM);
}

#include "mc_motifiupac.inc"
#include "mc_motifiter.inc"
#include "mc_motifprofile.inc"

// Everything behind the uploads.  d_text[0, n): the bed's text, a newline if it lacked its last, the control's from off2 on; padded.
// max_motifs: 0, or --iterative's
int ms_run(mc_ctx *c, Pool &pool, MsArgs &A, MsHead *d_head, const mc_motif_params &P, const std::vector<MsTable> &tables, bool iupac,
           int max_motifs, size_t scratch, const char **out, int64_t *n_out, int64_t *n_rows, int32_t *status) {
    mc_motif_stats &S = c->motif.stats;
    hipStream_t st = c->stream;
    const auto t_first = std::chrono::steady_clock::now();
    MsHead h = {};
    hipLaunchKernelGGL(km_pack, dim3((unsigned)(A.n_words * 64 / 256 + (A.n_words * 64 % 256 ? 1 : 0))), dim3(256), 0, st, A);
    if (A.n_contigs > 0) hipLaunchKernelGGL(km_contigs, dim3(blocks(A.n_contigs)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (A.n_bytes > 0) {
        long long *tile_off = nullptr, *line_start = nullptr;
        if (int rc = lines_count(pool, st, A.text, A.n_bytes, &d_head->kp, &tile_off)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.table_full) return ms_decline(c, status, MC_MOTIF_DECLINE_TABLE, 0, -1);
        A.n_nl = h.kp.n_newlines;
        if (too_many_lines(A.n_nl)) return ms_decline(c, status, MC_MOTIF_DECLINE_ROWS, 0, -1);
        if (!ms_fits(((size_t)A.n_nl + 2) * 8 + ((size_t)1 << 20))) return ms_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        if (int rc = lines_starts(pool, st, A.text, A.n_bytes, A.n_nl, tile_off, &d_head->kp, &line_start)) return rc;
        A.line_start = line_start;
        hipLaunchKernelGGL(km_parse, dim3(blocks(A.n_nl + 2)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(km_figures, dim3(blocks(A.n_words)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.table_full) return ms_decline(c, status, MC_MOTIF_DECLINE_TABLE, 0, -1);
    if (A.n_bytes > 0) {
        S.n_lines1 = h.n_lines1; S.n_lines2 = h.kp.n_lines - h.n_lines1;
        if (h.decline != MS_NO_DECLINE) return ms_decline_head(c, status, h);
    }
    S.n_candidates = (int64_t)h.n_candidates; S.n_sites = (int64_t)h.n_sites; S.n_control = (int64_t)h.n_control;
    S.n_off_base = (int64_t)h.n_off_base;
    // the counts: a launch per table, its histogram in LDS where that pays
    const unsigned n_stretch = (unsigned)((A.G + A.stretch - 1) / A.stretch);
    S.n_stretches = n_stretch;
    for (size_t t = 0; t < tables.size(); ++t) {
        const bool in_lds = (int64_t)tables[t].entries <= 2 * A.stretch;
        if (in_lds) {
            hipLaunchKernelGGL(km_count<true>, dim3(n_stretch), dim3(256), (size_t)tables[t].entries * 4, st, A, (int)t);
            ++S.n_tables_lds;
        } else {
            hipLaunchKernelGGL(km_count<false>, dim3(n_stretch), dim3(256), 0, st, A, (int)t);
            ++S.n_tables_global;
        }
    }
    HIP_TRY(hipGetLastError());
    if (max_motifs > 0) return it_run(c, pool, A, d_head, P, tables, iupac, max_motifs, scratch, t_first, out, n_out, n_rows, status);
    auto t_d2h = std::chrono::steady_clock::now();
    MsText text;
    int64_t NR = 0;
    if (iupac) {
        MiState mi;
        std::vector<MiPat> rows;
        if (int rc = mi_setup(pool, A, tables, scratch, mi)) return rc;
        if (int rc = mi_rows(c, pool, mi, tables, false, rows, &t_d2h, status)) return rc;
        if (*status != 0 || rows.empty()) return 0;
        for (const MiPat &r : rows)
            if (!mi_line(text, P, tables, r)) return ms_decline(c, status, MC_MOTIF_DECLINE_PRINT, 0, -1);
        NR = (int64_t)rows.size();
    } else {
        std::vector<MsRow> rows;
        if (int rc = ms_rows(c, pool, A, d_head, false, rows, &t_d2h, status)) return rc;
        if (*status != 0 || rows.empty()) return 0;
        for (const MsRow &r : rows)
            if (!ms_line(text, P, tables, r)) return ms_decline(c, status, MC_MOTIF_DECLINE_PRINT, 0, -1);
        NR = (int64_t)rows.size();
    }
    if (int rc = ms_hand_out(c, text, t_d2h, out, n_out)) return rc;
    *n_rows = NR;
    return 0;
}

// max_motifs: 0, or --iterative's 1 .. MC_MOTIF_MAX_ROUNDS
int ms_call(mc_ctx *c, const mc_ref_view *ref, const mc_text_source &s1, const mc_text_source *s2, const mc_motif_params *P, bool iupac,
            int max_motifs, const char **out, int64_t *n_out, int64_t *n_rows, int32_t *status) {
    mc_motif_stats &S = c->motif.stats;
    const auto blank = [&] { *out = nullptr; *n_out = 0; *n_rows = 0; c->motif.left_words = 0; };
    return pipeline_call(c, S, status, "motif finder", (size_t)32 << 20, blank, [&](Call &K) -> int {
        Pool &pool = K.pool;
        S.n_bytes1 = s1.n_bytes; S.n_bytes2 = s2 ? s2->n_bytes : 0;
        c->motif.iupac_stats = mc_motif_iupac_stats();
        c->motif.iter_stats = mc_motif_iter_stats();
        c->motif.iter_stats.decline_line = -1;
        c->motif.left_starts.clear();
        std::vector<MsTable> tables;
        std::vector<MsParent> parents;
        const int base_code = P->base == 'A' ? 0 : P->base == 'C' ? 1 : P->base == 'G' ? 2 : P->base == 'T' ? 3 : -1;
        if (base_code < 0 || !ms_tables(*P, tables, parents) || !(P->min_fraction >= 0.0) || P->min_sites < 0) {
            mc_set_error("mc_motif_report: a base other than A, C, G, T, a string that is no shape, or a negative threshold");
            return -12;
        }
        const int NC = ref->n_contigs;
        int64_t n_bases = 0;
        for (int i = 0; i < NC; ++i) n_bases += ref->contig_len[i];
        if (n_bases >= ((int64_t)1 << 31) || NC >= (1 << 24)) return ms_decline(c, status, MC_MOTIF_DECLINE_REFERENCE, 0, -1);
        // where the contigs stand: multiples of 64, at least 32 bases of padding behind each, 64 in front of the first
        std::vector<int64_t> gstart((size_t)NC + 1);
        int64_t G = 64;
        for (int i = 0; i < NC; ++i) {
            gstart[i] = G;
            G = (G + ref->contig_len[i] + 32 + 63) & ~(int64_t)63;
        }
        const int64_t n_words = G / 64 + 2;
        const uint32_t n_entries = tables.back().off + tables.back().entries;
        const int64_t n_text = s1.n_bytes + (s2 ? s2->n_bytes : 0);
        const int64_t id_bytes = NC > 0 ? P->contig_id_off[NC] : 0;
        const char *hs = getenv("MCALLER_MOTIF_STRETCH");
        int64_t stretch = hs && atoll(hs) >= 64 ? (atoll(hs) + 63) & ~63ll : MS_STRETCH;      // (below 64: as if unset)
        stretch = std::min<int64_t>(stretch, G);
        S.stretch = stretch; S.n_entries = n_entries;
        const uint64_t slots = table_slots(NC, 64, "MCALLER_MOTIF_TABLE_SLOTS");
        S.table_slots = (int64_t)slots;
        const size_t need = (size_t)ref->n_seq_bytes + (size_t)n_words * 8 * 9 + (size_t)n_entries * 14 + (size_t)n_text + (size_t)id_bytes +
                            (size_t)NC * 32 + slots * 8 + parents.size() * sizeof(MsParent) + ((size_t)1 << 20);
        size_t scratch = 0;
        const size_t need_iupac = iupac ? mi_need(tables, &scratch) : 0;    // (and the tables learn their places in the lattice block)
        c->motif.iupac_stats.lattice_bytes = (int64_t)need_iupac;
        const size_t need_iter = max_motifs > 0 ? it_need(n_bases, n_words, &c->motif.iter_stats.list_bytes) : 0;
        c->motif.iter_stats.need_bytes = (int64_t)(need + need_iupac + need_iter);
        if (!ms_fits(need + need_iupac + need_iter)) return ms_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        hipStream_t up = c->up_stream;
        MsArgs A = {};
        uint8_t *d_seq = nullptr;
        int64_t *d_meta = nullptr, *d_id_off = nullptr;
        char *d_ids = nullptr, *d_text = nullptr;
        uint64_t *d_planes = nullptr;
        MsTable *d_tables = nullptr;
        MsParent *d_parents = nullptr;
        MsHead *d_head = nullptr;
        if (pool.get(&d_seq, (size_t)ref->n_seq_bytes + 1) || pool.get(&d_meta, (size_t)NC * 3 + 1) || pool.get(&d_id_off, (size_t)NC + 1) ||
            pool.get(&d_ids, (size_t)id_bytes + 1) || pool.get(&d_text, (size_t)n_text + 1 + 64) || pool.get(&d_planes, (size_t)n_words * 9) ||
            pool.get(&d_tables, tables.size()) || pool.get(&d_parents, parents.size() + 1) || pool.get(&d_head, 1) ||
            pool.get(&A.nG, (size_t)n_entries * 3) || pool.get(&A.selected, (size_t)n_entries * 2))
            return -10;
        if (max_motifs > 0) {
            if (pool.get(&A.list, (size_t)n_bases + 1) || pool.get(&A.left, (size_t)n_words * 2)) return -10;
            A.cap_list = n_bases;
        }
        if (int rc = table_get(pool, up, &A.table, slots)) return rc;
        // the reference and the tables (pageable host memory: the copies are done when the calls return), then the texts
        std::vector<int64_t> meta((size_t)NC * 3 + 1);
        for (int i = 0; i < NC; ++i) { meta[i] = ref->contig_len[i]; meta[NC + i] = ref->seq_off[i]; meta[2 * NC + i] = gstart[i]; }
        MsHead h = {};
        h.decline = MS_NO_DECLINE;
        if (ref->n_seq_bytes > 0) HIP_TRY(hipMemcpyAsync(d_seq, ref->seq, (size_t)ref->n_seq_bytes, hipMemcpyHostToDevice, up));
        if (NC > 0) {
            HIP_TRY(hipMemcpyAsync(d_meta, meta.data(), (size_t)NC * 3 * 8, hipMemcpyHostToDevice, up));
            HIP_TRY(hipMemcpyAsync(d_id_off, P->contig_id_off, ((size_t)NC + 1) * 8, hipMemcpyHostToDevice, up));
            if (id_bytes > 0) HIP_TRY(hipMemcpyAsync(d_ids, P->contig_ids, (size_t)id_bytes, hipMemcpyHostToDevice, up));
        }
        HIP_TRY(hipMemcpyAsync(d_tables, tables.data(), tables.size() * sizeof(MsTable), hipMemcpyHostToDevice, up));
        if (!parents.empty()) HIP_TRY(hipMemcpyAsync(d_parents, parents.data(), parents.size() * sizeof(MsParent), hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemsetAsync(d_planes + 5 * n_words, 0, (size_t)n_words * 4 * 8, up));             // methylated and control, both strands
        HIP_TRY(hipMemsetAsync(A.nG, 0, (size_t)n_entries * 3 * 4, up));
        HIP_TRY(hipStreamSynchronize(up));                                // (meta, h and the vectors are the host's again)
        int64_t off2 = 0;
        if (int rc = K.feed.put_pair(s1, s2, d_text, &off2)) return rc;
        const int64_t n_bytes = s2 ? off2 + s2->n_bytes : s1.n_bytes;
        K.feed.times(S, K.t0);
        A.seq = d_seq; A.contig_len = d_meta; A.seq_off = d_meta + NC; A.gstart = d_meta + 2 * NC;
        A.n_contigs = NC; A.base_code = base_code; A.n_words = n_words;
        A.code0 = d_planes; A.code1 = d_planes + n_words; A.valid = d_planes + 2 * n_words;
        A.cand[0] = d_planes + 3 * n_words; A.cand[1] = d_planes + 4 * n_words;
        A.meth[0] = (unsigned long long *)(d_planes + 5 * n_words); A.meth[1] = (unsigned long long *)(d_planes + 6 * n_words);
        A.ctl[0] = (unsigned long long *)(d_planes + 7 * n_words); A.ctl[1] = (unsigned long long *)(d_planes + 8 * n_words);
        A.ids = d_ids; A.id_off = d_id_off; A.table_mask = slots - 1;
        const char *hm = getenv("MCALLER_MOTIF_HASH_MASK");
        A.hash_mask = hm && *hm ? strtoull(hm, nullptr, 16) : ~0ull;      // (tests: long probe chains)
        A.text = d_text; A.n_bytes = n_bytes; A.off2 = s2 ? off2 : n_bytes; A.head = d_head;
        A.tables = d_tables; A.parents = d_parents; A.n_tables = (int32_t)tables.size();
        A.has_control = s2 ? 1 : 0; A.keep_all = P->keep_all ? 1 : 0;
        A.stretch = stretch; A.G = G; A.n_entries = n_entries;
        A.nC = A.nG + n_entries; A.nM = A.nG + 2 * (size_t)n_entries;
        A.keep = A.selected + n_entries;
        A.min_sites = P->min_sites; A.min_fraction = P->min_fraction;
        const auto t_kernels = std::chrono::steady_clock::now();
        const int rc = ms_run(c, pool, A, d_head, *P, tables, iupac, max_motifs, scratch, out, n_out, n_rows, status);
        S.ms_kernels = ms_since(t_kernels) - S.ms_d2h;                     // a declined call too: what ran until it declined
        if (rc == 0 && *status == 0 && max_motifs > 0) c->motif.left_starts.assign(gstart.begin(), gstart.begin() + NC);
        return rc;
    });
}

bool ms_bad_args(const mc_ctx *c, const mc_ref_view *ref, const mc_motif_params *P, const char **out, int64_t *n_out, int64_t *n_rows,
                 int32_t *status) {
    if (!c || !ref || !P || !out || !n_out || !n_rows || !status || ref->n_contigs < 0) return true;
    if (ref->n_contigs > 0 && (!ref->contig_len || !ref->seq_off || !P->contig_id_off || !P->contig_ids)) return true;
    if (ref->n_seq_bytes < 0 || (ref->n_seq_bytes > 0 && !ref->seq)) return true;
    for (int i = 0; i < ref->n_contigs; ++i)
        if (ref->contig_len[i] < 0 || ref->seq_off[i] < 0 || ref->seq_off[i] + ref->contig_len[i] > ref->n_seq_bytes ||
            P->contig_id_off[i + 1] < P->contig_id_off[i] || P->contig_id_off[0] != 0)
            return true;
    return false;
}

}  // namespace

extern "C" int mc_motif_report(mc_ctx *c, const mc_ref_view *ref, const mc_text_source *bed, const mc_text_source *control,
                               const mc_motif_params *params, int32_t iupac, int32_t max_motifs, const char **out, int64_t *n_out,
                               int64_t *n_rows, int32_t *status) {
    if (ms_bad_args(c, ref, params, out, n_out, n_rows, status) || max_motifs < 0 || max_motifs > MC_MOTIF_MAX_ROUNDS) {
        mc_set_error("mc_motif_report: bad arguments");
        return -12;
    }
    mc_text_source s1 = {}, s2 = {};
    if (int rc = text_source("mc_motif_report", bed, &s1)) return rc;
    if (control)
        if (int rc = text_source("mc_motif_report", control, &s2)) return rc;
    const int rc = ms_call(c, ref, s1, control ? &s2 : nullptr, params, iupac != 0, max_motifs, out, n_out, n_rows, status);
    // the decline, if any, in the stats of --iupac and --iterative too (an iterative call fills both)
    const mc_motif_stats &S = c->motif.stats;
    if (iupac || max_motifs > 0) {
        mc_motif_iupac_stats &I = c->motif.iupac_stats;
        I.decline_line = S.decline_line; I.decline_reason = S.decline_reason; I.decline_file = S.decline_file;
    }
    if (max_motifs > 0) {
        mc_motif_iter_stats &I = c->motif.iter_stats;
        I.decline_line = S.decline_line; I.decline_reason = S.decline_reason; I.decline_file = S.decline_file;
    }
    return rc;
}

extern "C" int mc_motif_report_last_stats(mc_ctx *c, mc_motif_stats *out) {
    return stats_out("mc_motif_report_last_stats", c, out, &mc_ctx::motif, &MotifPipe::stats);
}

extern "C" int mc_motif_report_iupac_last_stats(mc_ctx *c, mc_motif_iupac_stats *out) {
    return stats_out("mc_motif_report_iupac_last_stats", c, out, &mc_ctx::motif, &MotifPipe::iupac_stats);
}

extern "C" int mc_motif_report_iter_last_stats(mc_ctx *c, mc_motif_iter_stats *out) {
    return stats_out("mc_motif_report_iter_last_stats", c, out, &mc_ctx::motif, &MotifPipe::iter_stats);
}

extern "C" int mc_motif_report_iter_left(mc_ctx *c, const uint64_t **plus, const uint64_t **minus, int64_t *n_words, const int64_t **contig_start,
                                         int32_t *n_contigs) {
    if (!c || !plus || !minus || !n_words || !contig_start || !n_contigs) { mc_set_error("mc_motif_report_iter_left: bad arguments"); return -12; }
    const bool have = c->motif.left_words > 0 && c->motif.left.get<uint64_t>();
    *plus = have ? c->motif.left.get<uint64_t>() : nullptr;
    *minus = have ? c->motif.left.get<uint64_t>() + c->motif.left_words : nullptr;
    *n_words = have ? c->motif.left_words : 0;
    *contig_start = have && !c->motif.left_starts.empty() ? c->motif.left_starts.data() : nullptr;
    *n_contigs = have ? (int32_t)c->motif.left_starts.size() : 0;
    return 0;
}

extern "C" int mc_motif_report_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::motif); }

extern "C" int mc_motif_profile(mc_ctx *c, const mc_ref_view *ref, const mc_text_source *bed, const mc_text_source *control,
                                const mc_motif_profile_params *params, mc_motif_profile_result *result, int32_t *status) {
    if (!c || !ref || !result || !status || mq_bad_params(params) || ref->n_contigs < 0 ||
        (ref->n_contigs > 0 && (!ref->contig_len || !ref->seq_off || !params->contig_id_off || !params->contig_ids)) || ref->n_seq_bytes < 0 ||
        (ref->n_seq_bytes > 0 && !ref->seq)) {
        mc_set_error("mc_motif_profile: bad arguments");
        return -12;
    }
    for (int i = 0; i < ref->n_contigs; ++i)
        if (ref->contig_len[i] < 0 || ref->seq_off[i] < 0 || ref->seq_off[i] + ref->contig_len[i] > ref->n_seq_bytes ||
            params->contig_id_off[i + 1] < params->contig_id_off[i] || params->contig_id_off[0] != 0) {
            mc_set_error("mc_motif_profile: bad arguments");
            return -12;
        }
    mc_text_source s1 = {}, s2 = {};
    if (int rc = text_source("mc_motif_profile", bed, &s1)) return rc;
    if (control)
        if (int rc = text_source("mc_motif_profile", control, &s2)) return rc;
    return mq_call(c, ref, s1, control ? &s2 : nullptr, params, result, status);
}

extern "C" int mc_motif_profile_last_stats(mc_ctx *c, mc_motif_profile_stats *out) {
    return stats_out("mc_motif_profile_last_stats", c, out, &mc_ctx::motif, &MotifPipe::profile_stats);
}

extern "C" int mc_motif_profile_release(mc_ctx *c) {
    if (!c) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    c->motif.release_profile();
    c->text_stages.release();
    return 0;
}
