// mc_bedsum.hip -- the per-site summary of a `.diffs.<k>` file on the GPU: what make_bed.py:67-164 writes for BED, BED --control,
// BED --vo and GFF, with a positions source for -p, with site_stats for --gff --vo and a FASTA source for --ref (C ABI:
// mc_bed_summarise, mc_bed_last_stats, mc_bed_release; Python: Device.bed_summarise, make_bed.summarise_diffs_device).  The unit stands in csrc/bed/,
// beside the units of the passes, not among them: no pass runs
// its kernels, and the benchmark's kernel hash (bench.KERNEL_SOURCES) names the files of the pass path one by one.
//
// Everything here is exact by construction -- integer counts, byte comparisons, one fp64 division whose quotient is printed by the
// digit generation of mc_rowtext.h -- or the call declines and the host code does the file (status 1, mc_last_error):
//   * a byte >= 0x80; a control byte other than tab and newline (0x7f too; '\r': Python's universal newlines split there)
//   * a line that is not 7 or 8 tab-separated fields (an empty line is one)
//   * a position that is not 1-9 decimal digits (int() accepts more forms; the end column is the integer + 1)
//   * an empty context or an empty label (the reference's IndexError)
//   * a 7-field row together with --vo
//   * a line longer than 65535 bytes (field offsets inside a line are 16 bits)
//   * 2^31 - 2 lines or more (rows and entries are numbered in 32 bits; a slot of the table holds row + 1)
//   * a table with fewer than 2 x the counted rows' slots (only MCALLER_BED_TABLE_SLOTS makes one)
//   * a text that does not fit into free device memory beside its tables: the WHOLE text stays resident, entries are compared
//     against the bytes of a representative row and the output copies its fields from there
//   * --gff with --vo without mc_bed_params.site_stats: not attempted (site_stats makes it, below)
//
// make_bed -p (mc_bed_summarise's positions source; Device.bed_summarise(positions_path= / positions_text=), make_bed.summarise_diffs_device(
// positions=); from the command line with MCALLER_BED_POSITIONS_DEVICE=1): a positions file beside the rows.  A row counts when its
// context has 'M' at its centre AND (chrom, pos text, digits of pos + 1, strand) is a tuple of the file, byte for byte; every entry
// is written, -d / -t / --control select nothing; a BED row carries two more columns before the --vo list, str(np.round(., 3)) of
// the largest t statistic and of the sum of -log10 p of one-sample t-tests of every value column of field 5 but the last
// ("nan" twice at depth 1); --gff writes the ordinary attributes.  The two numbers are not exact by construction, so every one comes
// with a bound on |device - host| (mc_tstat.h: the moments' part derived, the tail function's part measured against SciPy), and
// a value whose bound reaches a rounding tie declines the FILE -- exact bytes or a decline, never a guess.  More declines:
//   * positions file: a byte >= 0x80; a control byte other than tab and newline; a line longer than 65535 bytes
//   * a counted row with a value mc_decimal.h declines (nan, inf, blanks, more than 19 digits); with fewer than two values; with more
//     than MC_BED_MAX_VALUES; with another number of values than the first counted row
//   * an entry of depth >= 2 with a column without spread (the host prints inf / nan, and max() over NaNs depends on the order); a
//     log10 p below -290; a rounded value of 1e9 or more (mc_rowtext.h does not print it; "-0.0" it does); more than 100001 rows
//     (the tail function is measured up to 10^5 degrees of freedom); the tie test
// Its steps (mc_posset.inc, mc_sitestats.inc):
//   kq_parse / kq_insert   the positions file: line starts by kp_*, a lane per line (the `len(line) > 3` rule, strip, the first four
//                 fields, their KeyHash), a key table (mc_textdev.h); MCALLER_BED_HASH_MASK applies
//   kb_parse      probes that table for a row with a centre 'M' (the digits of pos + 1 are generated into the hash); an unwanted row is
//                 not counted and its values are never looked at; a counted row's commas are counted
//   kq_counts     every counted row has the first one's number of values
//   kb_sums .. kb_sort_*   every entry selected, every entry's bucket in ascending row order (the --vo machinery)
//   kq_features   a lane per NUMBER: mc_decimal.h into an fp64 matrix in bucket order
//   kq_moments_small / _large   per (entry, column) the mean and the centred sum of squares, compensated (two-sum), in an order the
//                 row order alone fixes: up to BS_SMALL rows a lane, more a wave (lane l the rows l, l + 64, ...; a fixed tree)
//   kq_finish     a lane per entry: t, log10 p, their bounds, the maximum and the sum, np.round(., 3), the tie test, the digits
//   kb_sums / kb_apply again (the rows' sizes with the two columns), kb_write
//
// make_bed --gff --vo and --ref (mc_bed_params.site_stats, mc_bed_summarise's FASTA source; Device.bed_summarise(site_stats=, ref_path= / ref_text=),
// make_bed.summarise_diffs_device(ref=); from the command line with MCALLER_BED_GFF_DEVICE=1, with -p both knobs).  --gff --vo: every
// written entry carries ";fracLow=..;fracUp=..;identificationQv=.." -- frac -+ 2 np.std(p, ddof=1) / np.sqrt(n) and int(100 np.mean(p))
// of its probabilities in row order, every fp64 operation with NumPy's two operands (mc_npsum.h: the pairwise order of np.add.reduce,
// a square root rounded in integers), so the values are the host's bits and nothing is bounded.  --ref: the FASTA text beside the
// rows; an entry's context in the GFF attributes is seq[p - 20 : p + 21] of its contig, upper-cased, on '-' complemented and
// reversed (a BED row keeps its own).  More declines:
//   * a row of a written entry with a probability mc_decimal.h declines (nan, inf, more than 19 digits, an exponent out of range)
//   * a fracLow / fracUp mc_rowtext.h does not print (0.0 and nan are printed); |100 * mean| >= 2^53
//   * FASTA: a byte >= 0x80; a control byte other than tab and newline ('\r' too); a sequence line of a record with a byte that is
//     no letter (the host strips blanks and keeps the rest: left to it); a text that does not fit beside the rest
//   * an entry on '-' whose window holds a letter outside ACGTNM (written or not: the host's KeyError); a written entry whose contig
//     the FASTA lacks (the host's KeyError, with and without --gff)
// Its steps (mc_gffstats.inc, mc_fastactx.inc; each file's head says more):
//   kf_lines / kp_scan x 2 / kf_pack / kf_ids   the FASTA: titles, ids and their hashes, the sequences packed upper-cased, a table of ids
//                 in which the LAST record of an id wins (atomicMax)
//   kf_context    behind kb_group, a lane per entry: the table probed with the chrom bytes, the slice rule, the letters on '-'
//   kb_sums .. kb_sort_*   as for --vo: every entry's bucket in ascending row order
//   kg_probs      a lane per row of a selected entry: the stripped probability text into fp64, in bucket order
//   kg_moments_small / _large   the mean and the sum of the rounded squares: up to 128 rows a lane (one leaf of NumPy's recursion),
//                 more a workgroup (thread k is node k of the tree of a chunk of 8192; the chunks joined in order)
//   kg_finish     a lane per entry: the three values, the digits -- or the decline
//   kb_sums / kb_apply again (the rows' sizes with the attributes), kb_write (no list: --gff writes none)
//
// The steps (one lane per line unless said otherwise; n = lines):
//   kp_count / kp_scan / kp_starts   line starts (the device parser's kernels: mc_lines.h, launched by mc_textfeed.h)
//   kb_parse      256 lines of a workgroup through LDS (staged_lines); per line: the class of every byte, the tabs, centre 'M',
//                 label 'm', the position as an integer, the stripped span of the probability, the KeyHash of the key fields.
//                 A flagged line: line_flag
//   kb_group      the keys into a table (kt_claim; ids are rows).  The row that claimed the slot numbers the entry; depth, n_meth,
//                 bytes of probabilities: atomicAdd, smallest row: atomicMin -- integers, so the result does not depend on the
//                 order of arrival.  Nothing crosses workgroups but these atomics.  longest_probe: slots that held another key
//   kb_sums / kp_scan / kb_apply   a row is its entry's head when it is the entry's smallest row.  Over the lines, exclusive
//                 scans of: depth at heads (an entry's bucket in rank order), selected heads, bytes of selected heads' text
//   kb_place / kb_sort_small / kb_sort_large (--vo)   rows into their entry's bucket (atomicAdd), then every selected bucket into
//                 ascending row order: up to 32 rows by insertion (one lane), more by a workgroup's LSD radix sort, 8 bits a
//                 pass, stable scatter chunk by chunk -- linear in the depth
//   kb_write / kb_write_vo   a lane per selected entry writes the columns (fields copied from the head row's spans, pos + 1 and
//                 the depth from the integers, the fraction from its digits); a wave per selected entry writes the list
// wave64; no library sort; every buffer, event and stream through the owners of mc_own.h.
// The host side around the kernels -- a file's way onto the device through the context's two pinned stages, the line starts, the
// head's way back, the decline, the clock, a key table's size -- is mc_textfeed.h's, and line_flag, ByteClass, KeyHash, kt_claim /
// kt_find, tabs_pack / tabs_unpack and staged_lines are mc_textdev.h's: shared with the other units that take a whole text file.
#include "../mc_textfeed.h"
#include "../mc_rowtext.h"
#include "../mc_decimal.h"
#include "../mc_tstat.h"
#include "../mc_hypergeom.h"
#include "../mc_npsum.h"

namespace {

constexpr int BS_STAGE = 48 * 1024;          // LDS a workgroup of kb_parse stages its 256 lines in (two workgroups share a CU's 160 KB)
constexpr int BS_SMALL = 32;                 // buckets up to this depth are sorted by insertion
constexpr uint8_t BS_F_COUNTED = 1, BS_F_METH = 2, BS_F_PROB = 4;
constexpr uint32_t BS_META_NAN = 1u << 20;   // a statistic the host prints as "nan" (beside the bits of rt_num_pack)

struct BsHead {                              // device-side result block (copied to the host as it is)
    KpHead kp;                               // n_newlines (kp_scan), n_lines (kp_starts)
    unsigned long long decline;              // min over the flagged lines of line << 8 | reason (~0: none)
    unsigned long long n_counted, n_entries;
    long long tot_bucket, tot_sel, tot_bytes;     // totals of the three scans
    unsigned int n_large;
    int longest_probe;
    unsigned long long first_counted;        // -p: the smallest counted line (~0: none)
    int nv, pad;                             // -p: values per row (kq_counts)
    unsigned int g_n_large, pad2;            // --gff --vo: entries deeper than a leaf (kg_moments_small)
    long long f_total, f_nrec;               // --ref: sequence bytes, records (the two scans over the FASTA's lines)
};

struct BsArgs {
    const char *text;
    int64_t n_bytes, n_lines, n_nl;
    const long long *line_start;
    BsHead *head;
    // per line
    uint4 *row;                              // tabs_pack: the tabs of a line (t[6] = len in a 7-field row), its length
    uint32_t *pos, *pspan, *row_ent, *ent_boff;
    uint64_t *hash;
    uint8_t *fl;
    // per entry, indexed by the row that claimed its slot
    uint32_t *ent_depth, *ent_meth, *ent_min, *ent_fill;
    unsigned long long *ent_pbytes;
    unsigned long long *table;
    uint64_t table_mask, hash_mask;
    long long min_depth;
    double thresh;
    int control, with_probs, gff;
    long long *blk_sum, *blk_off;            // [3 * nblk] each
    int64_t nblk;
    // per selected entry
    uint32_t *sel_line, *large;
    long long *sel_off, *sel_vo_at;
    uint32_t *bucket, *bucket_tmp;
    char *out;
    // -p (mc_posset.inc, mc_sitestats.inc)
    int positions;                           // rows are wanted by the position set; every entry is written
    int stats;                               // ... and a BED row carries the two statistics columns (not with --gff)
    int stats_ready;                         // the statistics are made: the sizing and writing kernels count and print them
    int buckets;                             // the rows of every entry are wanted in row order (--vo, or the statistics)
    const char *ptext;
    int64_t p_bytes, p_lines, p_nl;
    const long long *p_start;
    uint4 *p_line;
    uint64_t *p_hash;
    unsigned long long *p_table;
    uint64_t p_mask;
    uint32_t *nval;                          // per line: comma-separated values of field 5
    int nv;
    double *X, *mom;                         // [n_counted][nv] in bucket order; [n_sel][nv - 1][3]
    uint64_t *st_lo;                         // per entry (by the row that claimed its slot) x 2: the digits of the two values
    uint32_t *st_meta;
    // --gff --vo (mc_gffstats.inc): X holds the probabilities in bucket order, mom [n_sel][2] the mean and the sum of the squares,
    // st_lo / st_meta the digits of fracLow and fracUp
    int gstats;                              // the three attributes are wanted (then stats_ready says they are made)
    int vo_list;                             // a BED row ends with the list of probabilities (--vo without --gff)
    uint32_t *g_large;
    double *g_qv;                            // per entry: 100 * mean
    // --ref (mc_fastactx.inc)
    int ref;
    const char *ftext;
    int64_t f_bytes, f_lines, f_nl;
    const long long *f_start;
    long long *f_cnt, *f_off;                // [2 * f_lines] each: sequence bytes / titles of a line; their exclusive scans
    uint8_t *f_bad;
    uint32_t *f_idb, *f_idn;                 // per line: a title's id (offset from the line start, length)
    uint64_t *f_hash;
    char *f_seq;                             // the packed sequences, upper-cased
    long long n_rec;
    long long *rec_begin;                    // [n_rec + 1]
    uint32_t *rec_line;
    unsigned long long *f_table;
    uint32_t *f_win;                         // per slot: the last record of the id + 1
    uint64_t f_mask;
    long long *ctx_at;                       // per entry: where its window begins in f_seq
    uint8_t *ctx_len;                        // ... its length, bit 7: reversed and complemented
};

#include "mc_posset.inc"

// One line: t[x - adj] is byte x of the text (the staged piece in LDS, or the text itself with adj = 0: one address space per call site)
__device__ __forceinline__ bool bs_parse_line(const BsArgs &A, const char *t, const int64_t adj, const int64_t li) {
    const int64_t b = A.line_start[li] - adj;
    const int64_t e = (li < A.n_nl ? A.line_start[li + 1] - 1 : A.n_bytes) - adj;        // the newline, or the end of the text
    A.fl[li] = 0;
    if (e - b > 65535) { line_flag(&A.head->decline, li, MC_BED_DECLINE_LONG_LINE); return false; }
    const int len = (int)(e - b);
    int tab[7] = {0, 0, 0, 0, 0, 0, 0}, nt = 0, commas = 0;
    ByteClass bad;
    KeyHash H;                                                // the key fields in the one pass over the line
    for (int i = 0; i < len; ++i) {
        const unsigned c = (unsigned char)t[b + i];
        bad.see(c);
        if (c == '\t') {
#pragma unroll
            for (int k = 0; k < 7; ++k) tab[k] = nt == k ? i : tab[k];
            if (nt < 6) H.sep();                              // (the tab before a probability is no part of the key)
            ++nt;
        } else if (nt == 0 || nt == 2 || nt == 3 || nt == 5) {     // chrom, pos, context, strand
            H.put((char)c);
        } else if (nt == 4) {
            commas += c == ',';
        }
    }
    int &t1 = tab[1], &t2 = tab[2], &t3 = tab[3], &t5 = tab[5], &t6 = tab[6];       // (names for the rules below)
    int reason = 0;
    uint32_t pos = 0;
    if (bad.hi) reason = MC_BED_DECLINE_HIGH_BYTE;
    else if (bad.ctrl) reason = MC_BED_DECLINE_CONTROL;
    else if (nt != 6 && nt != 7) reason = MC_BED_DECLINE_FIELDS;
    else {
        if (nt == 6) t6 = len;
        const int pn = t2 - t1 - 1;
        if (pn < 1 || pn > 9) reason = MC_BED_DECLINE_POSITION;
        else
            for (int i = t1 + 1; i < t2; ++i) {
                const unsigned d = (unsigned)((unsigned char)t[b + i]) - '0';
                if (d > 9u) reason = MC_BED_DECLINE_POSITION;
                pos = pos * 10u + d;
            }
        if (!reason && t3 - t2 - 1 < 1) reason = MC_BED_DECLINE_CONTEXT;
        if (!reason && t6 - t5 - 1 < 1) reason = MC_BED_DECLINE_LABEL;
        if (!reason && nt == 6 && A.with_probs) reason = MC_BED_DECLINE_NO_PROB;
    }
    if (reason) { line_flag(&A.head->decline, li, reason); return false; }
    const int cn = t3 - t2 - 1;
    bool counted = t[b + t2 + 1 + cn / 2] == 'M';
    if (counted && A.positions) counted = bq_wanted(A, t + b, tab[0], t1, t2, tab[4], t5, pos);      // an unwanted row: its values are never looked at
    if (counted && A.stats) {
        A.nval[li] = (uint32_t)commas + 1u;
        atomicMin(&A.head->first_counted, (unsigned long long)li);
    }
    const bool meth = t[b + t5 + 1] == 'm';
    int pb = len, pe = len;                                   // f[7].strip(): blanks are the only whitespace a line still holds
    if (nt == 7) {
        pb = t6 + 1;
        while (pb < pe && t[b + pb] == ' ') ++pb;
        while (pe > pb && t[b + pe - 1] == ' ') --pe;
    }
    A.row[li] = tabs_pack(tab, len);
    A.pos[li] = pos;
    A.pspan[li] = ((uint32_t)pb << 16) | (uint32_t)(pe - pb);
    A.hash[li] = H.done(A.hash_mask);
    A.fl[li] = (uint8_t)((counted ? BS_F_COUNTED : 0) | (meth ? BS_F_METH : 0) | (nt == 7 ? BS_F_PROB : 0));
    return counted;
}

__global__ __launch_bounds__(256) void kb_parse(BsArgs A) {
    bool counted = false;
    (void)staged_lines<BS_STAGE>(A.text, A.n_bytes, A.line_start, A.n_lines, A.n_nl,
                                 [&](const char *t, int64_t adj, int64_t li) { counted = bs_parse_line(A, t, adj, li); });
    const unsigned long long bal = __ballot(counted);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.head->n_counted, (unsigned long long)__popcll(bal));
}

__device__ __forceinline__ TabSpan bs_row(const BsArgs &A, int64_t li) { return tabs_unpack(A.row[li]); }

// (chrom, pos, strand, context) of lines a and b, byte for byte: chrom = [0, t0), pos and context = (t1, t3) with the tab between
// them at the same place, strand = (t4, t5)
__device__ __forceinline__ bool bs_same_key(const BsArgs &A, int64_t a, int64_t b) {
    const TabSpan Ra = bs_row(A, a), Rb = bs_row(A, b);
    if (Ra.t[0] != Rb.t[0] || Ra.t[2] - Ra.t[1] != Rb.t[2] - Rb.t[1] || Ra.t[3] - Ra.t[1] != Rb.t[3] - Rb.t[1] ||
        Ra.t[5] - Ra.t[4] != Rb.t[5] - Rb.t[4])
        return false;
    const char *ta = A.text + A.line_start[a], *tb = A.text + A.line_start[b];
    return same_bytes(ta, tb, Ra.t[0]) && same_bytes(ta + Ra.t[1] + 1, tb + Rb.t[1] + 1, Ra.t[3] - Ra.t[1] - 1) &&
           same_bytes(ta + Ra.t[4] + 1, tb + Rb.t[4] + 1, Ra.t[5] - Ra.t[4] - 1);
}

__global__ __launch_bounds__(256) void kb_group(BsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint8_t fl = li < A.n_lines ? A.fl[li] : (uint8_t)0;
    int probes = 0;                                           // slots that held another key
    if (fl & BS_F_COUNTED) {
        const uint64_t h = A.hash[li];
        const KtHit hit = kt_claim(A.table, A.table_mask, h, li, [&](int64_t r) { return A.hash[r] == h && bs_same_key(A, li, r); });
        const int64_t rep = hit.id;                           // the row that claimed the slot numbers the entry
        probes = (int)hit.looked - (hit.slot >= 0 ? 1 : 0);
        if (hit.slot < 0) {
            line_flag(&A.head->decline, li, MC_BED_DECLINE_TABLE);
            A.row_ent[li] = (uint32_t)li;                     // (an entry nobody counted: no head, whatever runs before the host looks)
        } else {
            A.row_ent[li] = (uint32_t)rep;
            atomicAdd(&A.ent_depth[rep], 1u);
            if (fl & BS_F_METH) atomicAdd(&A.ent_meth[rep], 1u);
            atomicMin(&A.ent_min[rep], (uint32_t)li);
            if (A.with_probs) atomicAdd(&A.ent_pbytes[rep], (unsigned long long)(A.pspan[li] & 0xffffu));
        }
    }
    for (int o = 32; o > 0; o >>= 1) probes = max(probes, __shfl_xor(probes, o));
    if ((threadIdx.x & 63) == 0 && probes > 0) atomicMax(&A.head->longest_probe, probes);
}

// depth >= d and (fraction >= t) != control, the fraction an fp64 quotient (make_bed.py:21-28,:135-138)
// (-p: every entry -- its rows were wanted, make_bed.py:110-114)
__device__ __forceinline__ bool bs_selected(const BsArgs &A, uint32_t rep) {
    const uint32_t depth = A.ent_depth[rep], meth = A.ent_meth[rep];
    return A.positions || ((long long)depth >= A.min_depth && (((double)meth / (double)depth >= A.thresh) != (A.control != 0)));
}

// The text of an entry, counted or stored: li its head row.  (--vo: the list itself is kb_write_vo's; *vo_at = where it begins)
template <class Sink>
__device__ __forceinline__ void bs_put_span(Sink &o, const char *__restrict__ p, int n) {
    for (int i = 0; i < n; ++i) o.put(p[i]);
}
template <class Sink>
__device__ __forceinline__ void bs_put_lit(Sink &o, const char *s) {
    for (; *s; ++s) o.put(*s);
}

#include "mc_fastactx.inc"

template <class Sink>
__device__ __forceinline__ void bs_put_entry(const BsArgs &A, Sink &o, int64_t li, uint32_t depth, uint32_t meth) {
    const TabSpan R = bs_row(A, li);
    const char *t = A.text + A.line_start[li];
    const RtNum frac = rt_num_of((double)meth / (double)depth);       // np.float64(n_meth) / np.float64(depth)
    const uint32_t end = A.pos[li] + 1u;                              // str(int(pos) + 1)
    bs_put_span(o, t, R.t[0]);
    o.put('\t');
    if (A.gff) {
        bs_put_lit(o, "kinModCall\tm6A\t");
        rt_put_uint(o, end); o.put('\t'); rt_put_uint(o, end);
        bs_put_lit(o, "\t10\t");
        bs_put_span(o, t + R.t[4] + 1, R.t[5] - R.t[4] - 1);
        bs_put_lit(o, "\t.\tcoverage=");
        rt_put_uint(o, depth);
        bs_put_lit(o, ";context=");
        if (A.ref) bs_put_context(A, o, A.row_ent[li]);                 // (--ref reaches the GFF attributes only: make_bed.py:142,:155)
        else bs_put_span(o, t + R.t[2] + 1, R.t[3] - R.t[2] - 1);
        bs_put_lit(o, ";IPDRatio=5;frac=");
        rt_put_num(o, frac);
        if (A.gstats && A.stats_ready) {
            const size_t at = 2 * (size_t)A.row_ent[li];
            ns_put_attributes(o, rt_num_unpack(A.st_lo[at], A.st_meta[at]), (A.st_meta[at] & BS_META_NAN) != 0,
                              rt_num_unpack(A.st_lo[at + 1], A.st_meta[at + 1]), (A.st_meta[at + 1] & BS_META_NAN) != 0, A.g_qv[A.row_ent[li]]);
        }
        return;
    }
    bs_put_span(o, t + R.t[1] + 1, R.t[2] - R.t[1] - 1);
    o.put('\t');
    rt_put_uint(o, end);
    o.put('\t');
    bs_put_span(o, t + R.t[2] + 1, R.t[3] - R.t[2] - 1);
    o.put('\t');
    rt_put_num(o, frac);
    o.put('\t');
    bs_put_span(o, t + R.t[4] + 1, R.t[5] - R.t[4] - 1);
    o.put('\t');
    rt_put_uint(o, depth);
    if (A.stats && A.stats_ready)
        for (int q = 0; q < 2; ++q) {                                  // str(np.round(., 3)) of the largest t and of the sum of -log10 p
            const uint32_t meta = A.st_meta[2 * (size_t)A.row_ent[li] + q];
            o.put('\t');
            if (meta & BS_META_NAN) bs_put_lit(o, "nan");
            else rt_put_num(o, rt_num_unpack(A.st_lo[2 * (size_t)A.row_ent[li] + q], meta));
        }
}

struct BsEnt { bool head, sel; uint32_t depth, meth, rep; long long bytes; };

__device__ __forceinline__ BsEnt bs_entry(const BsArgs &A, int64_t li, bool want_bytes) {
    BsEnt E;
    E.head = E.sel = false; E.depth = E.meth = E.rep = 0; E.bytes = 0;
    if (li >= A.n_lines || !(A.fl[li] & BS_F_COUNTED)) return E;
    E.rep = A.row_ent[li];
    if (A.ent_min[E.rep] != (uint32_t)li) return E;
    E.head = true;
    E.depth = A.ent_depth[E.rep];
    E.meth = A.ent_meth[E.rep];
    E.sel = bs_selected(A, E.rep);
    if (E.sel && want_bytes) {
        RtCount c;
        bs_put_entry(A, c, li, E.depth, E.meth);
        E.bytes = (long long)c.n + 1;                                  // the newline
        if (A.vo_list) E.bytes += 1 + (long long)A.ent_pbytes[E.rep] + ((long long)E.depth - 1);     // tab, texts, commas
    }
    return E;
}

// exclusive prefix of v over the workgroup's 256 threads; *total: the workgroup's sum
__device__ __forceinline__ long long bs_block_excl(long long v, long long *s_w, long long *total) {
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

__global__ __launch_bounds__(256) void kb_sums(BsArgs A) {
    __shared__ long long s_w[4];
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const BsEnt E = bs_entry(A, li, true);
    long long tot[3], heads;
    (void)bs_block_excl(E.head ? (long long)E.depth : 0, s_w, &tot[0]);
    (void)bs_block_excl(E.sel ? 1 : 0, s_w, &tot[1]);
    (void)bs_block_excl(E.bytes, s_w, &tot[2]);
    (void)bs_block_excl(E.head ? 1 : 0, s_w, &heads);
    if (threadIdx.x == 0) {
        for (int q = 0; q < 3; ++q) A.blk_sum[q * A.nblk + blockIdx.x] = tot[q];
        if (heads && !A.stats_ready) atomicAdd(&A.head->n_entries, (unsigned long long)heads);      // (-p sizes twice)
    }
}

__global__ __launch_bounds__(256) void kb_apply(BsArgs A) {
    __shared__ long long s_w[4];
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const BsEnt E = bs_entry(A, li, true);
    long long tot;
    const long long boff = A.blk_off[blockIdx.x] + bs_block_excl(E.head ? (long long)E.depth : 0, s_w, &tot);
    const long long k = A.blk_off[A.nblk + blockIdx.x] + bs_block_excl(E.sel ? 1 : 0, s_w, &tot);
    const long long at = A.blk_off[2 * A.nblk + blockIdx.x] + bs_block_excl(E.bytes, s_w, &tot);
    if (E.head && A.buckets) A.ent_boff[li] = (uint32_t)boff;
    if (E.sel) { A.sel_line[k] = (uint32_t)li; A.sel_off[k] = at; }
}

__global__ __launch_bounds__(256) void kb_place(BsArgs A) {
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= A.n_lines || !(A.fl[li] & BS_F_COUNTED)) return;
    const uint32_t rep = A.row_ent[li];
    const uint32_t k = atomicAdd(&A.ent_fill[rep], 1u);
    A.bucket[(size_t)A.ent_boff[A.ent_min[rep]] + k] = (uint32_t)li;
}

// a lane per selected entry: its bucket into ascending row order if it is small, else onto the list of kb_sort_large
__global__ __launch_bounds__(256) void kb_sort_small(BsArgs A, int64_t n_sel) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const uint32_t li = A.sel_line[k];
    const uint32_t depth = A.ent_depth[A.row_ent[li]];
    if (depth > (uint32_t)BS_SMALL) { A.large[atomicAdd(&A.head->n_large, 1u)] = (uint32_t)k; return; }
    uint32_t *b = A.bucket + A.ent_boff[li];
    for (uint32_t i = 1; i < depth; ++i) {
        const uint32_t v = b[i];
        uint32_t j = i;
        for (; j > 0 && b[j - 1] > v; --j) b[j] = b[j - 1];
        b[j] = v;
    }
}

// A workgroup per large bucket (taken in turn from the list): LSD radix sort, 8 bits a pass, between the bucket and its twin in
// bucket_tmp; an even number of passes, so the rows end where they began.  The scatter goes chunk by chunk of 256 rows in order and
// is stable: a row's place = the digit's base + rows of that digit in earlier waves of the chunk + those before it in its wave
__global__ __launch_bounds__(256) void kb_sort_large(BsArgs A, int n_pass) {
    __shared__ unsigned s_base[256];
    __shared__ unsigned s_wc[4][256];
    __shared__ unsigned s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n_large = A.head->n_large;
    for (unsigned q = blockIdx.x; q < n_large; q += gridDim.x) {
        const uint32_t li = A.sel_line[A.large[q]];
        const uint32_t depth = A.ent_depth[A.row_ent[li]];
        uint32_t *b0 = A.bucket + A.ent_boff[li], *b1 = A.bucket_tmp + A.ent_boff[li];
        for (int p = 0; p < n_pass; ++p) {
            const uint32_t *src = (p & 1) ? b1 : b0;
            uint32_t *dst = (p & 1) ? b0 : b1;
            const int sh = 8 * p;
            s_base[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < depth; i += 256) atomicAdd(&s_base[(src[i] >> sh) & 255u], 1u);
            __syncthreads();
            {                                                       // exclusive scan of the 256 counts
                const unsigned c = s_base[tid];
                unsigned incl = c;
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned u = __shfl_up(incl, o);
                    if (lane >= o) incl += u;
                }
                if (lane == 63) s_w[wave] = incl;
                __syncthreads();
                unsigned before = 0;
                for (int w = 0; w < wave; ++w) before += s_w[w];
                s_base[tid] = before + incl - c;
            }
            __syncthreads();
            for (uint32_t c0 = 0; c0 < depth; c0 += 256) {
                const uint32_t i = c0 + tid;
                const bool valid = i < depth;
                const uint32_t key = valid ? src[i] : 0u;
                const unsigned d = (key >> sh) & 255u;
                unsigned long long peers = __ballot(valid);         // lanes of the wave with a row of the same digit
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
                    unsigned at = s_base[d] + before_me;
                    for (int w = 0; w < wave; ++w) at += s_wc[w][d];
                    dst[at] = key;
                }
                __syncthreads();
                if (leader) atomicAdd(&s_base[d], (unsigned)__popcll(peers));
                __syncthreads();
            }
        }
        __syncthreads();
    }
}

#include "mc_sitestats.inc"
#include "mc_gffstats.inc"

__global__ __launch_bounds__(256) void kb_write(BsArgs A, int64_t n_sel) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sel) return;
    const uint32_t li = A.sel_line[k];
    const uint32_t rep = A.row_ent[li];
    const uint32_t depth = A.ent_depth[rep];
    RtStore o{A.out + A.sel_off[k]};
    bs_put_entry(A, o, li, depth, A.ent_meth[rep]);
    if (A.vo_list) {
        o.put('\t');
        A.sel_vo_at[k] = (long long)(o.p - A.out);
        o.p += (long long)A.ent_pbytes[rep] + ((long long)depth - 1);
    }
    o.put('\n');
}

// a wave per selected entry: the stripped probability texts of its rows in row order, joined by ','
__global__ __launch_bounds__(256) void kb_write_vo(BsArgs A, int64_t n_sel) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_sel) return;
    const uint32_t li = A.sel_line[k];
    const uint32_t depth = A.ent_depth[A.row_ent[li]];
    const uint32_t *b = A.bucket + A.ent_boff[li];
    long long at = A.sel_vo_at[k];
    for (uint32_t c0 = 0; c0 < depth; c0 += 64) {
        const uint32_t i = c0 + lane;
        const bool valid = i < depth;
        const uint32_t r = valid ? b[i] : 0u;
        const uint32_t ps = valid ? A.pspan[r] : 0u;
        const int n = valid ? (int)(ps & 0xffffu) + (i > 0 ? 1 : 0) : 0;
        int incl = n;
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        if (valid) {
            char *w = A.out + at + incl - n;
            if (i > 0) *w++ = ',';
            const char *s = A.text + A.line_start[r] + (ps >> 16);
            for (int j = 0; j < (int)(ps & 0xffffu); ++j) w[j] = s[j];
        }
        at += __shfl(incl, 63);
    }
}

const char *bs_reason_text(int reason) {
    switch (reason) {
    case MC_BED_DECLINE_HIGH_BYTE: return "a byte >= 0x80";
    case MC_BED_DECLINE_CONTROL: return "a control byte other than tab and newline";
    case MC_BED_DECLINE_FIELDS: return "a line that is not 7 or 8 tab-separated fields";
    case MC_BED_DECLINE_POSITION: return "a position that is not 1-9 decimal digits";
    case MC_BED_DECLINE_CONTEXT: return "an empty context";
    case MC_BED_DECLINE_LABEL: return "an empty label";
    case MC_BED_DECLINE_NO_PROB: return "a 7-field row together with --vo";
    case MC_BED_DECLINE_LONG_LINE: return "a line longer than 65535 bytes";
    case MC_BED_DECLINE_TABLE: return "the table has fewer than 2 x the counted rows' slots";
    case MC_BED_DECLINE_ROWS: return "more lines than rows are numbered for (2^31 - 2)";
    case MC_BED_DECLINE_MEMORY: return "the text and its tables do not fit into free device memory";
    case MC_BED_DECLINE_OPTIONS: return "--gff with --vo is not summarised on the device";
    case MC_BED_DECLINE_POS_HIGH_BYTE: return "the positions file has a byte >= 0x80";
    case MC_BED_DECLINE_POS_CONTROL: return "the positions file has a control byte other than tab and newline";
    case MC_BED_DECLINE_POS_LONG_LINE: return "the positions file has a line longer than 65535 bytes";
    case MC_BED_DECLINE_VALUE: return "a value that is not a plain decimal number of up to 19 digits";
    case MC_BED_DECLINE_FEW_VALUES: return "a row with fewer than two values";
    case MC_BED_DECLINE_MANY_VALUES: return "a row with more than 64 values";
    case MC_BED_DECLINE_VALUE_COUNT: return "rows with differing numbers of values";
    case MC_BED_DECLINE_ZERO_VARIANCE: return "a site with a value column without spread";
    case MC_BED_DECLINE_FAR_TAIL: return "a log10 p below -290";
    case MC_BED_DECLINE_PRINT_RANGE: return "a statistic of 1e9 or more";
    case MC_BED_DECLINE_ROUNDING_TIE: return "a statistic too close to a rounding tie of np.round(., 3) to vouch for its last digit";
    case MC_BED_DECLINE_DEPTH: return "a site of more than 100001 rows";
    case MC_BED_DECLINE_PROBABILITY: return "a probability that is not a plain decimal number of up to 19 digits";
    case MC_BED_DECLINE_STAT_RANGE: return "a fracLow or fracUp outside the range the device prints";
    case MC_BED_DECLINE_QV_RANGE: return "100 x the mean probability is 2^53 or more";
    case MC_BED_DECLINE_REF_HIGH_BYTE: return "the FASTA has a byte >= 0x80";
    case MC_BED_DECLINE_REF_CONTROL: return "the FASTA has a control byte other than tab and newline";
    case MC_BED_DECLINE_REF_SEQ_BYTE: return "the FASTA has a sequence line with a byte that is not a letter";
    case MC_BED_DECLINE_REF_LETTER: return "a site on '-' with a letter outside ACGTNM in its window of the FASTA";
    case MC_BED_DECLINE_REF_CONTIG: return "a written site on a contig the FASTA lacks";
    }
    return "unknown";
}

int bs_decline(mc_ctx *c, int32_t *status, int reason, long long line) {
    return decline(c->bed.stats, status, "summary", bs_reason_text(reason), reason, line);
}

int bs_decline_head(mc_ctx *c, int32_t *status, const BsHead &h) {
    return bs_decline(c, status, decline_reason(h.decline), decline_line(h.decline));
}

// the line starts of a text on the device (padded): *n_nl newlines, *n_lines lines, line_start[0 .. n_lines] (n > 0)
int bs_lines(Pool &pool, hipStream_t st, const char *d_text, int64_t n, BsHead *d_head, BsHead &h, long long **line_start, int64_t *n_nl,
             int64_t *n_lines, bool *too_many) {
    long long *tile_off = nullptr;
    *too_many = false;
    if (int rc = lines_count(pool, st, d_text, n, &d_head->kp, &tile_off)) return rc;
    if (int rc = fetch_head(st, d_head, h)) return rc;
    *n_nl = h.kp.n_newlines;
    if (too_many_lines(*n_nl) || !device_fits((size_t)(*n_nl + 2) * 8 + ((size_t)1 << 20))) { *too_many = true; return 0; }
    if (int rc = lines_starts(pool, st, d_text, n, *n_nl, tile_off, &d_head->kp, line_start)) return rc;
    // (the last line may lack its newline: the same count kp_starts makes; the last byte is not on the host, so it is asked for)
    if (int rc = fetch_head(st, d_head, h)) return rc;
    *n_lines = h.kp.n_lines;
    return 0;
}

// -p: the positions text (on the device, padded) into the table the row parser probes -> 0: go on; 1: declined
int bs_position_set(mc_ctx *c, Pool &pool, BsArgs &A, BsHead *d_head, BsHead &h, const char *d_ptext, int64_t pn, int32_t *status, int *rc) {
    hipStream_t st = c->stream;
    *rc = 0;
    A.ptext = d_ptext; A.p_bytes = pn; A.p_mask = 15;
    long long *p_start = nullptr;
    if (pn > 0) {
        bool too_many = false;
        if ((*rc = bs_lines(pool, st, d_ptext, pn, d_head, h, &p_start, &A.p_nl, &A.p_lines, &too_many))) return 1;
        if (too_many) { (void)bs_decline(c, status, MC_BED_DECLINE_ROWS, -1); return 1; }
    }
    A.p_start = p_start;
    const size_t pl = (size_t)std::max<int64_t>(A.p_lines, 1);
    const uint64_t slots = table_slots(A.p_lines, 16);
    if (!device_fits(pl * (16 + 8) + (size_t)slots * 8)) { (void)bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1); return 1; }
    if (pool.get(&A.p_line, pl) || pool.get(&A.p_hash, pl) || table_get(pool, st, &A.p_table, slots)) { *rc = -10; return 1; }
    A.p_mask = slots - 1;
    if (A.p_lines > 0) {
        const unsigned pb = (unsigned)((A.p_lines + 255) / 256);
        hipLaunchKernelGGL(kq_parse, dim3(pb), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kq_insert, dim3(pb), dim3(256), 0, st, A);
        if (fetch_head(st, d_head, h)) { *rc = -11; return 1; }
        c->bed.stats.kernel_bytes += 3 * pn + A.p_lines * (8 + 16 + 8) * 2 + (int64_t)slots * 8;
        if (h.decline != ~0ull) { (void)bs_decline_head(c, status, h); return 1; }
    }
    return 0;
}

// --ref: the FASTA text (on the device, padded) into the packed sequences and the table of ids -> 0: go on; 1: declined or failed
int bs_fasta(mc_ctx *c, Pool &pool, BsArgs &A, BsHead *d_head, BsHead &h, const char *d_ftext, int64_t fn, int32_t *status, int *rc) {
    hipStream_t st = c->stream;
    *rc = 0;
    A.ref = 1; A.ftext = d_ftext; A.f_bytes = fn; A.f_mask = 15;
    if (fn == 0) return 0;                                    // no record: every written entry lacks its contig
    long long *f_start = nullptr;
    bool too_many = false;
    if ((*rc = bs_lines(pool, st, d_ftext, fn, d_head, h, &f_start, &A.f_nl, &A.f_lines, &too_many))) return 1;
    if (too_many) { (void)bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1); return 1; }
    A.f_start = f_start;
    const size_t fl = (size_t)A.f_lines;
    if (!device_fits(fl * (4 * 8 + 1 + 4 + 4 + 8) + ((size_t)1 << 20))) { (void)bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1); return 1; }
    if (pool.get(&A.f_cnt, 2 * fl) || pool.get(&A.f_off, 2 * fl) || pool.get(&A.f_bad, fl) || pool.get(&A.f_idb, fl) || pool.get(&A.f_idn, fl) ||
        pool.get(&A.f_hash, fl)) { *rc = -10; return 1; }
    const unsigned wb = (unsigned)((A.f_lines + 3) / 4);
    hipLaunchKernelGGL(kf_lines, dim3(wb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.f_cnt, A.f_lines, A.f_off, &d_head->f_total);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)(A.f_cnt + fl), A.f_lines, A.f_off + fl, &d_head->f_nrec);
    if (fetch_head(st, d_head, h)) { *rc = -11; return 1; }
    c->bed.stats.kernel_bytes += 3 * fn + A.f_lines * 6 * 8;
    if (h.decline != ~0ull) { (void)bs_decline_head(c, status, h); return 1; }
    A.n_rec = h.f_nrec;
    const uint64_t slots = table_slots(A.n_rec, 16);
    if (!device_fits((size_t)h.f_total + (size_t)A.n_rec * 12 + (size_t)slots * 12 + ((size_t)1 << 20))) { (void)bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1); return 1; }
    if (pool.get(&A.f_seq, (size_t)h.f_total + 1) || pool.get(&A.rec_begin, (size_t)A.n_rec + 1) || pool.get(&A.rec_line, (size_t)A.n_rec + 1) ||
        pool.get(&A.f_win, (size_t)slots) || table_get(pool, st, &A.f_table, slots)) { *rc = -10; return 1; }
    A.f_mask = slots - 1;
    if (hipMemsetAsync(A.f_win, 0, (size_t)slots * 4, st) != hipSuccess) { *rc = -11; return 1; }
    hipLaunchKernelGGL(kf_pack, dim3(wb), dim3(256), 0, st, A, A.n_rec, h.f_total);
    if (A.n_rec > 0) hipLaunchKernelGGL(kf_ids, dim3((unsigned)((A.n_rec + 255) / 256)), dim3(256), 0, st, A, A.n_rec);
    if (fetch_head(st, d_head, h)) { *rc = -11; return 1; }
    c->bed.stats.kernel_bytes += fn + h.f_total + A.f_lines * 3 * 8 + A.n_rec * 40;
    if (h.decline != ~0ull) { (void)bs_decline_head(c, status, h); return 1; }
    return 0;
}

// The text is on the device (d_text[0, n), padded; copies enqueued on c->up_stream): everything behind that.  d_ptext: the
// positions text of -p (pn bytes, padded), or null; d_ftext: the FASTA text of --ref (fn bytes, padded), or null
int bs_run(mc_ctx *c, Pool &pool, const char *d_text, int64_t n, const char *d_ptext, int64_t pn, const char *d_ftext, int64_t fn,
           const mc_bed_params *P, const char **out, int64_t *n_out, int64_t *n_sites, int32_t *status) {
    mc_bed_stats &S = c->bed.stats;
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    const auto t_kernels = std::chrono::steady_clock::now();
    if (n == 0) return 0;                                     // no line, no entry: an empty file
    BsHead *d_head = nullptr, h = {};
    if (pool.get(&d_head, 1)) return -10;
    h.decline = ~0ull;
    h.first_counted = ~0ull;
    HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    BsArgs A = {};
    A.head = d_head;
    A.hash_mask = ~0ull;
    if (const char *e = getenv("MCALLER_BED_HASH_MASK")) A.hash_mask = strtoull(e, nullptr, 16);
    A.positions = d_ptext != nullptr;
    A.stats = A.positions && !P->gff;
    A.buckets = P->with_probs || A.stats;
    A.gstats = P->gff && P->with_probs;
    A.vo_list = P->with_probs && !P->gff;
    if (d_ftext) {
        int rc = 0;
        if (bs_fasta(c, pool, A, d_head, h, d_ftext, fn, status, &rc)) return rc;
        h.kp = KpHead();                                      // (the line passes count from zero again)
        HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    }
    if (A.positions) {
        int rc = 0;
        if (bs_position_set(c, pool, A, d_head, h, d_ptext, pn, status, &rc)) return rc;
        h.kp = KpHead();                                      // (the line passes count from zero again)
        HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, st));
    }
    long long *line_start = nullptr;
    int64_t n_nl = 0, n_lines = 0;
    bool too_many = false;
    if (int rc = bs_lines(pool, st, d_text, n, d_head, h, &line_start, &n_nl, &n_lines, &too_many)) return rc;
    if (too_many) return bs_decline(c, status, n_nl + 1 >= ((int64_t)1 << 31) - 2 ? MC_BED_DECLINE_ROWS : MC_BED_DECLINE_MEMORY, -1);
    // per line: the row, four 32-bit columns, the hash, the flags, the entry's five columns (-p: the value count, two numbers' digits)
    if (!device_fits((size_t)(n_nl + 2) * (16 + 4 * 4 + 8 + 1 + 4 * 4 + 8 + (A.stats ? 4 + 2 * 12 : 0) + (A.gstats ? 2 * 12 + 8 : 0) + (A.ref ? 9 : 0)) +
                 ((size_t)1 << 20)))
        return bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1);
    S.n_lines = n_lines;
    A.text = d_text; A.n_bytes = n; A.n_lines = n_lines; A.n_nl = n_nl; A.line_start = line_start;
    A.min_depth = P->min_depth; A.thresh = P->mod_threshold; A.control = P->control; A.with_probs = P->with_probs; A.gff = P->gff;
    const size_t nl = (size_t)n_lines;
    if (pool.get(&A.row, nl) || pool.get(&A.pos, nl) || pool.get(&A.pspan, nl) || pool.get(&A.row_ent, nl) || pool.get(&A.ent_boff, nl) ||
        pool.get(&A.hash, nl) || pool.get(&A.fl, nl) || pool.get(&A.ent_depth, nl) || pool.get(&A.ent_meth, nl) || pool.get(&A.ent_min, nl) ||
        pool.get(&A.ent_fill, nl) || pool.get(&A.ent_pbytes, nl))
        return -10;
    if (A.stats && (pool.get(&A.nval, nl) || pool.get(&A.st_lo, 2 * nl) || pool.get(&A.st_meta, 2 * nl))) return -10;
    if (A.gstats && (pool.get(&A.st_lo, 2 * nl) || pool.get(&A.st_meta, 2 * nl) || pool.get(&A.g_qv, nl))) return -10;
    if (A.ref) {
        if (pool.get(&A.ctx_at, nl) || pool.get(&A.ctx_len, nl)) return -10;
        HIP_TRY(hipMemsetAsync(A.ctx_at, 0, nl * 8, st));
        HIP_TRY(hipMemsetAsync(A.ctx_len, 0, nl, st));
    }
    const unsigned lb = (unsigned)((n_lines + 255) / 256);
    A.nblk = lb;
    hipLaunchKernelGGL(kb_parse, dim3(lb), dim3(256), BS_STAGE + 16, st, A);
    if (int rc = fetch_head(st, d_head, h)) return rc;
    S.kernel_bytes += 3 * n + n_lines * (8 + 16 + 4 + 4 + 8 + 1);       // the text: counted, split, parsed; the line columns
    if (h.decline != ~0ull) return bs_decline_head(c, status, h);
    const int64_t n_counted = (int64_t)h.n_counted;
    S.n_counted = n_counted;
    if (A.stats && n_counted > 0) {                           // every counted row has the first one's number of values, 2 .. 64
        hipLaunchKernelGGL(kq_counts, dim3(lb), dim3(256), 0, st, A);
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.decline != ~0ull) return bs_decline_head(c, status, h);
        A.nv = h.nv;
    }
    const uint64_t slots = table_slots(n_counted, 16, "MCALLER_BED_TABLE_SLOTS");
    S.table_slots = (int64_t)slots;
    if ((int64_t)slots < 2 * n_counted) return bs_decline(c, status, MC_BED_DECLINE_TABLE, -1);
    if (!device_fits((size_t)slots * 8 + (size_t)3 * lb * 16 + (A.buckets ? (size_t)n_counted * 8 : 0))) return bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1);
    if (pool.get(&A.blk_sum, (size_t)3 * lb) || pool.get(&A.blk_off, (size_t)3 * lb) || table_get(pool, st, &A.table, slots)) return -10;      // (cleared behind the last allocation)
    A.table_mask = slots - 1;
    HIP_TRY(hipMemsetAsync(A.ent_depth, 0, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.ent_meth, 0, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.ent_fill, 0, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.ent_min, 0xff, nl * 4, st));
    HIP_TRY(hipMemsetAsync(A.ent_pbytes, 0, nl * 8, st));
    hipLaunchKernelGGL(kb_group, dim3(lb), dim3(256), 0, st, A);
    if (A.ref) hipLaunchKernelGGL(kf_context, dim3(lb), dim3(256), 0, st, A);      // (before the sizes: an entry's text holds its window)
    // the three scans over the lines: bucket places, selected entries, bytes of text (-p with statistics: once more when they are made)
    auto size_entries = [&]() -> int {
        hipLaunchKernelGGL(kb_sums, dim3(lb), dim3(256), 0, st, A);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)A.blk_sum, (int64_t)lb, A.blk_off, &d_head->tot_bucket);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)(A.blk_sum + lb), (int64_t)lb, A.blk_off + lb, &d_head->tot_sel);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)(A.blk_sum + 2 * (size_t)lb), (int64_t)lb, A.blk_off + 2 * (size_t)lb,
                           &d_head->tot_bytes);
        if (int rc = fetch_head(st, d_head, h)) return rc;
        return 0;
    };
    if (int rc = size_entries()) return rc;
    S.kernel_bytes += (int64_t)slots * 8 + n_lines * 5 * 8 + n_counted * (16 + 8 + 5 * 4 + 60) + 2 * n_lines * (1 + 4 + 3 * 4);
    S.longest_probe = h.longest_probe;
    if (h.decline != ~0ull) return bs_decline_head(c, status, h);
    S.n_entries = (int64_t)h.n_entries;
    const int64_t n_sel = h.tot_sel;
    int64_t n_outb = h.tot_bytes;
    S.n_sites = n_sel;
    *n_sites = n_sel;
    if (n_sel > 0) {
        if (!device_fits((size_t)n_sel * 32 + (size_t)n_outb + (A.stats ? (size_t)n_counted * A.nv * 8 + (size_t)n_sel * A.nv * 24 : 0) +
                     (A.gstats ? (size_t)n_counted * 8 + (size_t)n_sel * 20 + (size_t)n_sel * 64 : 0)))
            return bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1);
        if (pool.get(&A.sel_line, (size_t)n_sel) || pool.get(&A.large, (size_t)n_sel) || pool.get(&A.sel_off, (size_t)n_sel) ||
            pool.get(&A.sel_vo_at, (size_t)n_sel))
            return -10;
        if (A.buckets && (pool.get(&A.bucket, (size_t)n_counted) || pool.get(&A.bucket_tmp, (size_t)n_counted))) return -10;
        const unsigned sb = (unsigned)((n_sel + 255) / 256);
        hipLaunchKernelGGL(kb_apply, dim3(lb), dim3(256), 0, st, A);
        if (A.buckets) {
            hipLaunchKernelGGL(kb_place, dim3(lb), dim3(256), 0, st, A);
            hipLaunchKernelGGL(kb_sort_small, dim3(sb), dim3(256), 0, st, A, n_sel);
            hipLaunchKernelGGL(kb_sort_large, dim3((unsigned)std::min<int64_t>(n_sel, 1024)), dim3(256), 0, st, A, n_lines <= 65536 ? 2 : 4);
        }
        if (A.stats) {
            const int64_t n_num = n_counted * A.nv, n_mom = n_sel * (A.nv - 1);
            if (pool.get(&A.X, (size_t)n_num) || pool.get(&A.mom, (size_t)n_mom * 3)) return -10;
            hipLaunchKernelGGL(kq_features, dim3((unsigned)((n_num + 255) / 256)), dim3(256), 0, st, A, n_num);
            if (int rc = fetch_head(st, d_head, h)) return rc;                            // (a value that is no number: named before the moments run on it)
            if (h.decline != ~0ull) return bs_decline_head(c, status, h);
            hipLaunchKernelGGL(kq_moments_small, dim3((unsigned)((n_mom + 255) / 256)), dim3(256), 0, st, A, n_sel);
            hipLaunchKernelGGL(kq_moments_large, dim3((unsigned)std::min<int64_t>((n_mom + 3) / 4, 4096)), dim3(256), 0, st, A);
            hipLaunchKernelGGL(kq_finish, dim3(sb), dim3(256), 0, st, A, n_sel);
            HIP_TRY(hipGetLastError());
            A.stats_ready = 1;                                // the rows' sizes with the two columns, and their places
            if (int rc = size_entries()) return rc;
            S.kernel_bytes += n_counted * 60 + 3 * n_num * 8 + 2 * n_mom * 24 + n_lines * (1 + 4 + 3 * 4);
            if (h.decline != ~0ull) return bs_decline_head(c, status, h);
            n_outb = h.tot_bytes;
            if (!device_fits((size_t)n_outb)) return bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1);
            hipLaunchKernelGGL(kb_apply, dim3(lb), dim3(256), 0, st, A);
        }
        if (A.gstats) {
            if (pool.get(&A.X, (size_t)n_counted) || pool.get(&A.mom, (size_t)n_sel * 2) || pool.get(&A.g_large, (size_t)n_sel)) return -10;
            hipLaunchKernelGGL(kg_probs, dim3((unsigned)((n_counted + 255) / 256)), dim3(256), 0, st, A, n_counted);
            if (int rc = fetch_head(st, d_head, h)) return rc;                            // (a text that is no number: named before the sums run on it)
            if (h.decline != ~0ull) return bs_decline_head(c, status, h);
            hipLaunchKernelGGL(kg_moments_small, dim3(sb), dim3(256), 0, st, A, n_sel);
            hipLaunchKernelGGL(kg_moments_large, dim3((unsigned)std::min<int64_t>(n_sel, 4096)), dim3(NS_NODES), 0, st, A);
            hipLaunchKernelGGL(kg_finish, dim3(sb), dim3(256), 0, st, A, n_sel);
            HIP_TRY(hipGetLastError());
            A.stats_ready = 1;                                // the rows' sizes with the three attributes, and their places
            if (int rc = size_entries()) return rc;
            S.kernel_bytes += n_counted * (60 + 3 * 8) + n_sel * 2 * (16 + 12) + n_lines * (1 + 4 + 3 * 4);
            if (h.decline != ~0ull) return bs_decline_head(c, status, h);
            n_outb = h.tot_bytes;
            if (!device_fits((size_t)n_outb)) return bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1);
            hipLaunchKernelGGL(kb_apply, dim3(lb), dim3(256), 0, st, A);
        }
        if (pool.get(&A.out, (size_t)n_outb)) return -10;
        hipLaunchKernelGGL(kb_write, dim3(sb), dim3(256), 0, st, A, n_sel);
        if (A.vo_list) hipLaunchKernelGGL(kb_write_vo, dim3((unsigned)((n_sel + 3) / 4)), dim3(256), 0, st, A, n_sel);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        S.kernel_bytes += n_lines * (1 + 4 + 3 * 4) + 2 * n_outb + (A.buckets ? n_counted * 24 : 0);
    }
    S.n_out_bytes = n_outb;
    S.ms_kernels = ms_since(t_kernels);
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = fetch_out(c, c->bed.out, A.out, (size_t)n_outb, out, n_out)) return rc;
    S.ms_d2h = ms_since(t_d2h);
    return 0;
}

// What the entry point runs: the texts of the sources, each padded in a buffer of its own, onto the device and through bs_run.
// pos == null -> no -p; fa == null -> no --ref
int bs_call(mc_ctx *c, const mc_text_source &src, const mc_text_source *pos, const mc_text_source *fa, const mc_bed_params *P,
            const char **out, int64_t *n_out, int64_t *n_sites, int32_t *status) {
    mc_bed_stats &S = c->bed.stats;
    return pipeline_call(c, S, status, "bed summary", (size_t)64 << 20, [&] { *out = nullptr; *n_out = 0; *n_sites = 0; }, [&](Call &K) -> int {
        const int64_t pn = pos ? pos->n_bytes : 0, fn = fa ? fa->n_bytes : 0;
        S.n_bytes = src.n_bytes + pn + fn;                    // (a call that declines here: the bytes of all its texts)
        // the options first: such a call declines before any device work
        if (P->gff && P->with_probs && !P->site_stats) return bs_decline(c, status, MC_BED_DECLINE_OPTIONS, -1);
        if (!device_fits((size_t)S.n_bytes + 4096)) return bs_decline(c, status, MC_BED_DECLINE_MEMORY, -1);
        S.n_bytes = src.n_bytes;
        char *d_text = nullptr, *d_ptext = nullptr, *d_ftext = nullptr;
        if (int rc = K.feed.put(K.pool, src, &d_text)) return rc;
        if (pos)
            if (int rc = K.feed.put(K.pool, *pos, &d_ptext)) return rc;
        if (fa)
            if (int rc = K.feed.put(K.pool, *fa, &d_ftext)) return rc;
        K.feed.times(S, K.t0);
        return bs_run(c, K.pool, d_text, src.n_bytes, d_ptext, pn, d_ftext, fn, P, out, n_out, n_sites, status);
    });
}

// the probe of mc_tstat.h's device build: a lane per triple
__global__ __launch_bounds__(256) void k_ts_probe(const double *__restrict__ n, const double *__restrict__ mean, const double *__restrict__ var,
                                                  int64_t count, double *__restrict__ t, double *__restrict__ l, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double tv, lv;
    status[i] = ts_stat(n[i], mean[i], var[i], &tv, &lv);
    t[i] = tv; l[i] = lv;
}

// the probe of mc_hypergeom.h's device build: a lane per case (bad arguments: NaN twice)
__global__ __launch_bounds__(256) void k_hg_probe(const long long *__restrict__ N, const long long *__restrict__ K, const long long *__restrict__ d,
                                                  const long long *__restrict__ k, int64_t count, double *__restrict__ tail, double *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double t, e;
    (void)hg_tail(N[i], K[i], d[i], k[i], &t, &e);
    tail[i] = t; err[i] = e;
}

}  // namespace

extern "C" int mc_bed_summarise(mc_ctx *c, const mc_text_source *src, const mc_text_source *positions, const mc_text_source *fasta,
                                const mc_bed_params *P, const char **out, int64_t *n_out, int64_t *n_sites, int32_t *status) {
    if (!c || !P || !out || !n_out || !n_sites || !status) {
        mc_set_error("mc_bed_summarise: bad arguments");
        return -12;
    }
    mc_text_source s = {}, pos = {}, fa = {};
    if (int rc = text_source("mc_bed_summarise", src, &s)) return rc;
    if (positions)
        if (int rc = text_source("mc_bed_summarise", positions, &pos)) return rc;
    if (fasta)
        if (int rc = text_source("mc_bed_summarise", fasta, &fa)) return rc;
    return bs_call(c, s, positions ? &pos : nullptr, fasta ? &fa : nullptr, P, out, n_out, n_sites, status);
}

// p: the arrays one behind the other, off[count + 1] their places; out6 per array: fracLow, fracUp, 100 * mean, mean, var, se
extern "C" int mc_gff_site_stats_device(mc_ctx *c, const double *p, const int64_t *off, const double *frac, int64_t count, double *out6,
                                        int32_t *status) {
    if (!c || count < 0 || (count > 0 && (!p || !off || !frac || !out6 || !status))) {
        mc_set_error("mc_gff_site_stats_device: bad arguments");
        return -12;
    }
    if (count == 0) return 0;
    for (int64_t i = 0; i < count; ++i)
        if (off[i + 1] <= off[i] || off[0] != 0) { mc_set_error("mc_gff_site_stats_device: an empty array"); return -12; }
    HIP_TRY(hipSetDevice(c->device));
    Pool pool("site statistics probe");
    const int64_t total = off[count];
    double *d_p = nullptr, *d_frac = nullptr, *d_out = nullptr;
    long long *d_off = nullptr;
    int32_t *d_st = nullptr;
    if (pool.get(&d_p, (size_t)total) || pool.get(&d_off, (size_t)count + 1) || pool.get(&d_frac, (size_t)count) || pool.get(&d_out, (size_t)count * 6) ||
        pool.get(&d_st, (size_t)count))
        return -10;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_p, p, (size_t)total * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, off, ((size_t)count + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_frac, frac, (size_t)count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ns_probe, dim3((unsigned)std::min<int64_t>(count, 4096)), dim3(NS_NODES), 0, st, (const double *)d_p, (const long long *)d_off,
                       (const double *)d_frac, count, d_out, d_st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out6, d_out, (size_t)count * 48, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_st, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mc_npsum_se_device(mc_ctx *c, const double *var, const double *n, int64_t count, double *se) {
    if (!c || count < 0 || (count > 0 && (!var || !n || !se))) {
        mc_set_error("mc_npsum_se_device: bad arguments");
        return -12;
    }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Pool pool("standard error probe");
    double *d_in = nullptr, *d_out = nullptr;
    if (pool.get(&d_in, (size_t)count * 2) || pool.get(&d_out, (size_t)count)) return -10;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_in, var, (size_t)count * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_in + count, n, (size_t)count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ns_se_probe, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double *)d_in, (const double *)(d_in + count), count, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(se, d_out, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mc_tstat_device(mc_ctx *c, const double *n, const double *mean, const double *var, int64_t count, double *t, double *log10_p,
                               int32_t *status) {
    if (!c || count < 0 || (count > 0 && (!n || !mean || !var || !t || !log10_p || !status))) {
        mc_set_error("mc_tstat_device: bad arguments");
        return -12;
    }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Pool pool("t statistic probe");
    double *d_in = nullptr, *d_out = nullptr;
    int32_t *d_st = nullptr;
    if (pool.get(&d_in, (size_t)count * 3) || pool.get(&d_out, (size_t)count * 2) || pool.get(&d_st, (size_t)count)) return -10;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(d_in, n, (size_t)count * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_in + count, mean, (size_t)count * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_in + 2 * count, var, (size_t)count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ts_probe, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double *)d_in, (const double *)(d_in + count),
                       (const double *)(d_in + 2 * count), count, d_out, d_out + count, d_st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t, d_out, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(log10_p, d_out + count, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, d_st, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mc_hypergeom_tail_device(mc_ctx *c, const int64_t *N, const int64_t *K, const int64_t *d, const int64_t *k, int64_t count, double *tail,
                                        double *err) {
    if (!c || count < 0 || (count > 0 && (!N || !K || !d || !k || !tail || !err))) {
        mc_set_error("mc_hypergeom_tail_device: bad arguments");
        return -12;
    }
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Pool pool("hypergeometric tail probe");
    long long *d_in = nullptr;
    double *d_out = nullptr;
    if (pool.get(&d_in, (size_t)count * 4) || pool.get(&d_out, (size_t)count * 2)) return -10;
    hipStream_t st = c->stream;
    const int64_t *in[4] = {N, K, d, k};
    for (int q = 0; q < 4; ++q) HIP_TRY(hipMemcpyAsync(d_in + q * count, in[q], (size_t)count * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hg_probe, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const long long *)d_in, (const long long *)(d_in + count),
                       (const long long *)(d_in + 2 * count), (const long long *)(d_in + 3 * count), count, d_out, d_out + count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tail, d_out, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(err, d_out + count, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mc_bed_last_stats(mc_ctx *c, mc_bed_stats *out) { return stats_out("mc_bed_last_stats", c, out, &mc_ctx::bed, &BedPipe::stats); }

extern "C" int mc_bed_release(mc_ctx *c) { return release_pipeline(c, &mc_ctx::bed); }
