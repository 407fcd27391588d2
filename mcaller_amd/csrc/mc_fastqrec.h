// mc_fastqrec.h -- the rules of a FASTQ record as read_qual.py:15-47 states them, once, for a host and a device compiler alike
// (plain integer code).  The host build: mc_fastq_records_host (mc_fastq.cpp), sequential, no GPU; the device build: the kernels of
// fastq/mc_fastqual.hip.  tests/test_fastq_records.py holds the host build against read_qual.extract_read_quality_py, and
// tests/test_gpu_fastq.py the device build against both.
//
// Lines: a line ends at '\n'; a '\r' directly before that '\n' belongs to the line break; a last line without '\n' ends at the end
// of the text.  line_start[0] = 0, line_start[1 + j] = the offset behind the j-th newline (n_nl newlines; mc_lines.h on the
// device).  A line index at or beyond the lines the text has is an empty line.
// Records: `last` = the last line with a byte other than blank and tab; R = last / 4 + 1 records (no such line: none); record r
// is lines 4r .. 4r + 3.  Whitespace-only lines behind `last` are ignored; everywhere else a line is what its place says:
//   line 4r      byte 0 is '@' (a blank line there is a decline: the host reader skips it, this reader counts in fours); the id is
//                the first run of bytes behind the '@' that are not blank or tab (none: a decline); the key is the id up to its
//                first ':' or '_' (it may be empty)
//   line 4r + 2  byte 0 is '+' (so `last` mod 4 is 2 or 3: with 0 or 1 the last record's third line is empty)
//   line 4r + 3  as long as line 4r + 1 without its leading and trailing blanks and tabs
// Bytes: >= 0x80, a control byte other than tab, '\n' and '\r', 0x7f, and a '\r' not directly followed by '\n' are declines.
// Of several offending lines the first is named, of several reasons on one line the smallest: min of line << 8 | reason.
// The mean: double(sum of the quality bytes - 33 n) / double(n), one IEEE division of exact integers; NaN for n = 0.
#pragma once
#include <stdint.h>

#include "../../include/mcaller_hip.h"

#if defined(__HIP__)
#define FQ_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define FQ_HD inline
#endif

#define FQ_PIECE 4096               // bytes of a quality line one wave sums (fastq/mc_fastqual.hip: kfq_sum)
#define FQ_NO_DECLINE (~0ull)

struct FqRecord {
    int64_t key_b, key_n;           // the key's bytes: text[key_b, key_b + key_n)
    int64_t qual_b, qual_n;         // the quality line's
    int64_t seq_n;                  // the sequence line's length, stripped
};

FQ_HD bool fq_blank(unsigned c) { return c == ' ' || c == '\t'; }

FQ_HD unsigned long long fq_code(int64_t line, int reason) { return ((unsigned long long)line << 8) | (unsigned long long)reason; }

// why byte c, followed by byte `next` (-1: the end of the text), makes the reader decline -> 0, or MC_FASTQ_DECLINE_*
FQ_HD int fq_byte_reason(unsigned c, int next) {
    if (c >= 0x80u) return MC_FASTQ_DECLINE_HIGH_BYTE;
    if ((c < 0x20u && c != '\t' && c != '\n' && c != '\r') || c == 0x7fu) return MC_FASTQ_DECLINE_CONTROL;
    if (c == '\r' && next != '\n') return MC_FASTQ_DECLINE_LONE_CR;
    return 0;
}

// ---- four bytes at a time: bit 7 of every byte of a little-endian word that ... ----
FQ_HD uint32_t fq_eq_bits(uint32_t v, uint32_t c) {          // ... equals c (c < 0x80)
    v ^= c * 0x01010101u;
    const uint32_t t = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | v | 0x7F7F7F7Fu);
}
FQ_HD uint32_t fq_lt20_bits(uint32_t v) {                    // ... is below 0x20
    return ~(((v & 0x7F7F7F7Fu) + 0x60606060u) | v) & 0x80808080u;
}
// ... is >= 0x80, a control byte other than tab, '\n' and '\r', or 0x7f; *cr: is '\r'; *nl: is '\n'; *fill: is blank, tab, '\r' or '\n'
FQ_HD uint32_t fq_bad_bits(uint32_t v, uint32_t *cr, uint32_t *nl, uint32_t *fill) {
    const uint32_t tab = fq_eq_bits(v, '\t');
    *cr = fq_eq_bits(v, '\r');
    *nl = fq_eq_bits(v, '\n');
    *fill = tab | *cr | *nl | fq_eq_bits(v, ' ');
    return (v & 0x80808080u) | (fq_lt20_bits(v) & ~(tab | *cr | *nl)) | fq_eq_bits(v, 0x7fu);
}

// the span of line li without its line break
template <typename Off>
FQ_HD void fq_line_span(const char *text, int64_t n_bytes, const Off *line_start, int64_t n_nl, int64_t n_lines, int64_t li, int64_t *b,
                        int64_t *e) {
    if (li >= n_lines) { *b = *e = n_bytes; return; }
    *b = (int64_t)line_start[li];
    if (li < n_nl) {
        *e = (int64_t)line_start[li + 1] - 1;
        if (*e > *b && text[*e - 1] == '\r') --*e;
    } else {
        *e = n_bytes;
    }
}

// the line that holds byte `off`: the last one that starts at or before it
template <typename Off>
FQ_HD int64_t fq_line_of(const Off *line_start, int64_t n_nl, int64_t off) {
    int64_t lo = 0, hi = n_nl;                                // (line_start[0 .. n_nl] are valid, line_start[0] = 0 <= off)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if ((int64_t)line_start[mid] <= off) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Record r from the spans [b[i], e[i]) of its four lines -> 0, or the decline's code (fq_code of the offending line and the reason).
// Reads the title line, the two ends of the sequence line and byte 0 of the third line; of the quality line only the span.
FQ_HD unsigned long long fq_record(const char *text, int64_t r, const int64_t *b, const int64_t *e, FqRecord *out) {
    out->key_b = b[0]; out->key_n = 0; out->qual_b = b[3]; out->qual_n = 0; out->seq_n = 0;
    if (e[0] <= b[0] || text[b[0]] != '@') return fq_code(4 * r, MC_FASTQ_DECLINE_TITLE);
    int64_t ib = b[0] + 1;
    while (ib < e[0] && fq_blank((unsigned char)text[ib])) ++ib;
    if (ib == e[0]) return fq_code(4 * r, MC_FASTQ_DECLINE_EMPTY_ID);
    int64_t ke = ib;
    while (ke < e[0] && !fq_blank((unsigned char)text[ke]) && text[ke] != ':' && text[ke] != '_') ++ke;
    out->key_b = ib; out->key_n = ke - ib;
    if (e[2] <= b[2] || text[b[2]] != '+') return fq_code(4 * r + 2, MC_FASTQ_DECLINE_PLUS);
    int64_t sb = b[1], se = e[1];
    while (sb < se && fq_blank((unsigned char)text[sb])) ++sb;
    while (se > sb && fq_blank((unsigned char)text[se - 1])) --se;
    out->seq_n = se - sb;
    if (e[3] - b[3] != se - sb) return fq_code(4 * r + 3, MC_FASTQ_DECLINE_LENGTH);
    out->qual_n = e[3] - b[3];
    return 0;
}

// (host only) the words of a decline in mc_last_error
inline const char *fq_reason_text(int reason) {
    switch (reason) {
    case MC_FASTQ_DECLINE_HIGH_BYTE: return "a byte >= 0x80";
    case MC_FASTQ_DECLINE_CONTROL: return "a control byte other than tab and the line breaks";
    case MC_FASTQ_DECLINE_LONE_CR: return "a carriage return that no newline follows";
    case MC_FASTQ_DECLINE_TITLE: return "a title line that does not start with '@' (blank lines between records are the host reader's)";
    case MC_FASTQ_DECLINE_PLUS: return "a record whose third line does not start with '+'";
    case MC_FASTQ_DECLINE_LENGTH: return "a quality line and a sequence line of different lengths";
    case MC_FASTQ_DECLINE_EMPTY_ID: return "a title line without a read id";
    case MC_FASTQ_DECLINE_ROWS: return "more lines than are numbered (2^31 - 2)";
    case MC_FASTQ_DECLINE_MEMORY: return "the text and its outputs do not fit into free device memory";
    case MC_FASTQ_DECLINE_GZ: return "a gzip-compressed file";
    }
    return "unknown";
}

FQ_HD double fq_mean(uint64_t byte_sum, int64_t n) {
    if (n == 0) return __builtin_nan("");
    return (double)((int64_t)byte_sum - 33 * n) / (double)n;
}
