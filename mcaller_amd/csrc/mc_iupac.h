// mc_iupac.h -- the rule of a degenerate (IUPAC) motif set, once, for a host and a device compiler alike (plain integer code).
// The host build: mc_mark_iupac (mc_common.cpp), sequential, no GPU; the device build: k_ref_planes / k_mark_iupac
// (mc_devparse.inc).  tests/test_iupac_motifs.py holds the host build against a brute-force restatement (tests/iupac_sites.py),
// tests/test_gpu_iupac_motifs.py the device build against the host build.
//
// Letters: ACGT RYSWKM BDHV N, each a set over A, C, G, T (bits 1, 2, 4, 8).  M in a motif is {A, C}, not the mark letter.
// Matching: a sequence byte matches a motif letter iff it is one of A C G T (upper case) and lies in the letter's set; every
// other byte -- N, an IUPAC letter, a literal M -- matches nothing.
// '+' strand: position q + j is marked for every called offset j (0-based) of the motif and every start q at which the whole
// motif matches inside the contig; every occurrence counts, overlapping ones included.  '-' strand: the same for the reverse
// complement of the motif (sets complemented, order reversed) with the called offsets mirrored.  A literal 'M' of the
// sequence is marked on both strands.
#pragma once
#include <stdint.h>

#include "../../include/mcaller_hip.h"

#if defined(__HIP__)
#define IU_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define IU_HD inline
#endif

#define IU_A 1u
#define IU_C 2u
#define IU_G 4u
#define IU_T 8u

// the set of an upper-case motif letter; 0: no IUPAC letter
IU_HD unsigned iu_letter_set(unsigned c) {
    switch (c) {
    case 'A': return IU_A;
    case 'C': return IU_C;
    case 'G': return IU_G;
    case 'T': return IU_T;
    case 'R': return IU_A | IU_G;
    case 'Y': return IU_C | IU_T;
    case 'S': return IU_C | IU_G;
    case 'W': return IU_A | IU_T;
    case 'K': return IU_G | IU_T;
    case 'M': return IU_A | IU_C;
    case 'B': return IU_C | IU_G | IU_T;
    case 'D': return IU_A | IU_G | IU_T;
    case 'H': return IU_A | IU_C | IU_T;
    case 'V': return IU_A | IU_C | IU_G;
    case 'N': return IU_A | IU_C | IU_G | IU_T;
    }
    return 0;
}

// the one-base set of an upper-case sequence byte; 0: matches nothing
IU_HD unsigned iu_base_bit(unsigned c) { return c == 'A' ? IU_A : c == 'C' ? IU_C : c == 'G' ? IU_G : c == 'T' ? IU_T : 0u; }

IU_HD unsigned iu_upper(unsigned c) { return (c >= 'a' && c <= 'z') ? c - 32u : c; }

// A <-> T, C <-> G: the four bits in reverse order
IU_HD unsigned iu_comp_set(unsigned s) { return ((s & 1u) << 3) | ((s & 2u) << 1) | ((s & 4u) >> 1) | ((s & 8u) >> 3); }

// Entry `at` of the spec from a motif's upper-case letters and its called offsets (bit j: letter j is called): the '+' table
// and the reverse complement's.  -> 0, or -1: a length outside 1..32, a letter that is none, no called letter, or a called bit
// beyond the motif
IU_HD int iu_set_entry(mc_iupac_spec *S, int at, const char *motif, int m, uint32_t called) {
    if (at < 0 || at >= MC_IUPAC_MAX_MOTIFS || m < 1 || m > MC_IUPAC_MAX_LEN || called == 0) return -1;
    if (m < 32 && (called >> m) != 0) return -1;
    mc_iupac_motif *F = &S->fwd[at], *R = &S->rev[at];
    F->m = R->m = m;
    F->called = called;
    R->called = 0;
    for (int i = 0; i < MC_IUPAC_MAX_LEN; ++i) F->set[i] = R->set[i] = 0;
    for (int i = 0; i < m; ++i) {
        const unsigned s = iu_letter_set((unsigned char)motif[i]);
        if (!s) return -1;
        F->set[i] = (uint8_t)s;
        R->set[m - 1 - i] = (uint8_t)iu_comp_set(s);
        if ((called >> i) & 1u) R->called |= 1u << (m - 1 - i);
    }
    return 0;
}

// is the spec one the marking may index by?  (1..8 motifs of 1..32 non-empty sets, called offsets inside the motif, on both strands)
IU_HD bool iu_spec_ok(const mc_iupac_spec *S) {
    if (!S || S->n_motifs < 1 || S->n_motifs > MC_IUPAC_MAX_MOTIFS) return false;
    for (int k = 0; k < 2 * S->n_motifs; ++k) {
        const mc_iupac_motif *M = k & 1 ? &S->rev[k >> 1] : &S->fwd[k >> 1];
        if (M->m < 1 || M->m > MC_IUPAC_MAX_LEN || M->called == 0 || (M->m < 32 && (M->called >> M->m) != 0)) return false;
        for (int i = 0; i < M->m; ++i)
            if (M->set[i] == 0 || M->set[i] > 15) return false;
    }
    return true;
}

// does motif M match the upper-case bytes s[q, q + M.m)?  (the caller keeps q + M.m inside the contig)
IU_HD bool iu_match_at(const mc_iupac_motif *M, const uint8_t *s, int64_t q) {
    for (int i = 0; i < M->m; ++i)
        if (!(iu_base_bit(s[q + i]) & M->set[i])) return false;
    return true;
}

// One strand of a contig, sequentially: out[0, n) already holds the upper-case sequence (a literal 'M' is a mark as it stands);
// every called offset of every occurrence of every motif of the table becomes 'M'.  Matching reads `upper`, never `out`.
IU_HD void iu_mark_strand(const mc_iupac_motif *table, int n_motifs, const uint8_t *upper, int64_t n, char *out) {
    for (int k = 0; k < n_motifs; ++k) {
        const mc_iupac_motif *M = &table[k];
        for (int64_t q = 0; q + M->m <= n; ++q) {
            if (!iu_match_at(M, upper, q)) continue;
            for (int j = 0; j < M->m; ++j)
                if ((M->called >> j) & 1u) out[q + j] = 'M';
        }
    }
}

// ---- the same rule on bit-planes (bit b of a plane <=> the base at position p0 + b is that letter; zero outside the contig) ----
typedef unsigned __int128 iu_u128;

// the plane of a letter set: the OR of the planes of its bases
IU_HD iu_u128 iu_set_plane(unsigned set, iu_u128 a, iu_u128 c, iu_u128 g, iu_u128 t) {
    iu_u128 p = 0;
    if (set & IU_A) p |= a;
    if (set & IU_C) p |= c;
    if (set & IU_G) p |= g;
    if (set & IU_T) p |= t;
    return p;
}

// marks of one motif over a window of 128 positions: starts = AND over i of (plane of letter i >> i), marks = OR over the called
// j of (starts << j).  Exact for every position b of the window with b >= 31 whose occurrences' letters all lie below bit 128:
// a caller that wants the marks of bits [32, 64) loads [0, 96).
IU_HD iu_u128 iu_window_marks(const mc_iupac_motif *M, iu_u128 a, iu_u128 c, iu_u128 g, iu_u128 t) {
    iu_u128 starts = ~(iu_u128)0;
    for (int i = 0; i < M->m; ++i) starts &= iu_set_plane(M->set[i], a, c, g, t) >> i;
    iu_u128 marks = 0;
    for (int j = 0; j < M->m; ++j)
        if ((M->called >> j) & 1u) marks |= starts << j;
    return marks;
}
