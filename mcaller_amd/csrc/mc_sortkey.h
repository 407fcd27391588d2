// mc_sortkey.h -- what `sort -n -k2` compares first, as an order-preserving unsigned integer, for a host and a device compiler
// alike (mCaller.numeric_key_k2 is the yardstick).  C ABI: mc_sort_key (the host build, mc_format.cpp); the device build is
// km_key's (merge/mc_rowmerge.hip).  tests/test_sortkey.py holds the host build against Decimal.
//
// The grammar: field 1 ends at the first blank or tab; blanks and tabs behind it are skipped; then an optional '-', digits, and an
// optional '.' followed by at least one digit (a '.' with no digit behind it is no part of the number).  No digit at all: 0.
// The key is the pair (hi, lo), compared as one 128-bit unsigned number:
//   value >= 0:  hi = 2^63 + I,      lo = F          I: the integer part, leading zeros dropped (at most 18 digits: I < 10^18 < 2^60)
//   value <  0:  hi = 2^63 - 1 - I,  lo = ~F         F: the fraction's first 18 digits as an integer (trailing zeros change nothing)
// so -0, '-', 'abc' and an empty field all give (2^63, 0), 007 gives what 7 gives and 0.50 what .5 gives.
// Declined (-> 1): more than 18 significant integer digits, or a nonzero fraction digit behind the 18th.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define SK_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define SK_HD inline
#endif

#define SK_MAX_INT_DIGITS 18
#define SK_MAX_FRAC_DIGITS 18

// the key of the line s[0, n) (its newline may be among the bytes: it is no blank, digit, '-' or '.') -> 0, or 1: beyond the limits
SK_HD int sk_key(const unsigned char *s, int64_t n, uint64_t *hi, uint64_t *lo) {
    int64_t i = 0;
    while (i < n && s[i] != ' ' && s[i] != '\t') ++i;
    while (i < n && (s[i] == ' ' || s[i] == '\t')) ++i;
    bool neg = false;
    if (i < n && s[i] == '-') { neg = true; ++i; }
    while (i < n && s[i] == '0') ++i;
    uint64_t I = 0, F = 0;
    int nd = 0;
    for (; i < n && (unsigned)(s[i] - '0') <= 9u; ++i) {
        if (++nd > SK_MAX_INT_DIGITS) return 1;
        I = I * 10u + (uint64_t)(s[i] - '0');
    }
    if (i < n && s[i] == '.') {
        int nf = 0;
        for (++i; i < n && (unsigned)(s[i] - '0') <= 9u; ++i) {
            const unsigned d = (unsigned)(s[i] - '0');
            if (nf < SK_MAX_FRAC_DIGITS) { F = F * 10u + d; ++nf; }
            else if (d) return 1;
        }
        for (; nf < SK_MAX_FRAC_DIGITS; ++nf) F *= 10u;
    }
    if (!neg || (I == 0 && F == 0)) { *hi = (1ull << 63) + I; *lo = F; }
    else { *hi = (1ull << 63) - 1ull - I; *lo = ~F; }
    return 0;
}
