// mc_decimal.h -- decimal text -> double, correctly rounded, for a host and a device compiler alike: the inverse of mc_rowtext.h
// (which writes repr()'s digits).  C ABI: mc_parse_double (the host build, mc_format.cpp), mc_parse_doubles_device (a lane per
// token, train/mc_trainrows.hip); tests/test_decimal.py and tests/test_gpu_decimal.py hold both against Python's float().
//
// Accepted:  [+-]? digits? ('.' digits?)? ([eE] [+-]? digits)?  with at least one mantissa digit, and, once leading zeros are
// stripped and trailing zeros are folded into the exponent, a significand w of at most 19 digits (w < 10^19 < 2^64) and a decimal
// exponent q with |q| <= 27 (5^|q| < 2^63).  A zero significand is +-0.0 whatever the exponent.  Everything else float() accepts or
// rejects is DECLINED (-> 0), never guessed: surrounding whitespace, '_', inf / nan / infinity, more digits, exponents outside the
// range, the empty string, a bare '.', "e5", "1e", hex forms.  repr() of a double with 1e-7 <= |x| < 1e9 has at most 17 digits and
// an exponent of -23 at the least: always inside.
//
// Exact by construction: the value is (M + f) * 2^e with a 128-bit integer M of at least 55 bits, 0 <= f < 1 and `sticky` = (f != 0)
//   q >= 0:  M = w * 5^q (below 2^127: exact), e = q, f = 0
//   q <  0:  N = w shifted up until its highest bit is bit 127 (by s), M = N / 5^-q, the remainder is the sticky bit, e = q - s
//            (the divisor is below 2^63, so the quotient has 65 bits or more); the 128 / 64 division is done in limbs (dc_div128:
//            Knuth's algorithm D with 32-bit digits) -- no device runtime has a 128-bit division
// and M is rounded to 53 bits, half-way to even, in integers.  Every result is a normal double (1e-27 .. 1e46): no fp64
// operation takes part.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define DC_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define DC_HD inline
#endif

#define DC_MAX_DIGITS 19
#define DC_MAX_EXP10 27

DC_HD int dc_clz64(uint64_t x) { return __builtin_clzll(x); }           // x != 0

// (u1 : u0) / v for u1 < v -> the 64-bit quotient, *r the remainder (Knuth 4.3.1 D, two 32-bit quotient digits)
DC_HD uint64_t dc_div128(uint64_t u1, uint64_t u0, uint64_t v, uint64_t *r) {
    const uint64_t b = 1ull << 32;
    const int s = dc_clz64(v);
    v <<= s;
    const uint64_t vn1 = v >> 32, vn0 = v & 0xffffffffull;
    const uint64_t un32 = s ? (u1 << s) | (u0 >> (64 - s)) : u1;
    const uint64_t un10 = u0 << s;
    const uint64_t un1 = un10 >> 32, un0 = un10 & 0xffffffffull;
    uint64_t q1 = un32 / vn1, rhat = un32 - q1 * vn1;
    while (q1 >= b || q1 * vn0 > b * rhat + un1) {
        --q1; rhat += vn1;
        if (rhat >= b) break;
    }
    const uint64_t un21 = un32 * b + un1 - q1 * v;
    uint64_t q0 = un21 / vn1;
    rhat = un21 - q0 * vn1;
    while (q0 >= b || q0 * vn0 > b * rhat + un0) {
        --q0; rhat += vn1;
        if (rhat >= b) break;
    }
    *r = (un21 * b + un0 - q0 * v) >> s;
    return q1 * b + q0;
}

// (hi : lo + f) * 2^e, hi : lo != 0, sticky = (f != 0) -> the bits of the nearest double, half-way to even (a normal double: the
// caller's range)
DC_HD uint64_t dc_round(uint64_t hi, uint64_t lo, bool sticky, int e) {
    const int len = hi ? 128 - dc_clz64(hi) : 64 - dc_clz64(lo);          // bits of hi : lo
    uint64_t m;
    int sh = len - 53;                                                    // bits that go
    if (sh <= 0) {
        m = lo << -sh;                                                    // (len <= 53: hi == 0) exact
    } else {
        uint64_t rest, half;                                              // what goes, as a number below 2^64: its low bits folded into sticky
        if (sh <= 64) {
            m = sh == 64 ? hi : (hi << (64 - sh)) | (lo >> sh);
            rest = sh == 64 ? lo : lo << (64 - sh);                       // the bits that go, highest first
        } else {
            m = hi >> (sh - 64);
            rest = (hi << (128 - sh)) | (lo >> (sh - 64));
            sticky = sticky || (lo << (128 - sh)) != 0;
        }
        half = 1ull << 63;
        if (rest > half || (rest == half && (sticky || (m & 1ull)))) ++m;
        if (m == (1ull << 53)) { m >>= 1; ++sh; }
    }
    return ((uint64_t)(e + sh + 52 + 1023) << 52) | (m & 0xFFFFFFFFFFFFFull);
}

// w * 10^q, 0 < w < 10^19, |q| <= 27 -> the bits of the nearest double
DC_HD uint64_t dc_scale(uint64_t w, int q) {
    const uint64_t p5[DC_MAX_EXP10 + 1] = {1ull, 5ull, 25ull, 125ull, 625ull, 3125ull, 15625ull, 78125ull, 390625ull, 1953125ull, 9765625ull,
                                           48828125ull, 244140625ull, 1220703125ull, 6103515625ull, 30517578125ull, 152587890625ull,
                                           762939453125ull, 3814697265625ull, 19073486328125ull, 95367431640625ull, 476837158203125ull,
                                           2384185791015625ull, 11920928955078125ull, 59604644775390625ull, 298023223876953125ull,
                                           1490116119384765625ull, 7450580596923828125ull};
    if (q >= 0) {
        const unsigned __int128 m = (unsigned __int128)w * p5[q];
        return dc_round((uint64_t)(m >> 64), (uint64_t)m, false, q);
    }
    const uint64_t d = p5[-q];
    const int s = dc_clz64(w);
    const uint64_t n1 = w << s;                                           // N = n1 : 0 = w << (s + 64)
    const uint64_t qh = n1 / d;
    uint64_t rem;
    const uint64_t ql = dc_div128(n1 - qh * d, 0ull, d, &rem);
    return dc_round(qh, ql, rem != 0, q - s - 64);
}

// the token s[0, n) -> 1: *out is float(s), bit for bit; 0: declined (see above), *out untouched
DC_HD int dc_parse(const char *s, int n, double *out) {
    int i = 0;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; ++i; }
    uint64_t w = 0;
    int nd = 0;                      // digits of w
    int pz = 0, pz_frac = 0;         // zeros behind a non-zero digit that wait for the next one: all of them, those behind the point
    long long q = 0;                 // the decimal exponent the point's place gives
    bool any = false, frac = false, many = false;
    for (; i < n; ++i) {
        const unsigned c = (unsigned char)s[i];
        if (c == '.') {
            if (frac) return 0;
            frac = true;
            continue;
        }
        const unsigned d = c - '0';
        if (d > 9u) break;
        any = true;
        if (d == 0u) {
            if (nd == 0) q -= frac ? 1 : 0;                               // a leading zero
            else { ++pz; pz_frac += frac ? 1 : 0; }
            continue;
        }
        if (nd + pz + 1 > DC_MAX_DIGITS) { many = true; continue; }      // (the rest is still checked against the grammar)
        nd += pz + 1;
        for (; pz > 0; --pz) w *= 10u;
        w = w * 10u + d;
        q -= pz_frac + (frac ? 1 : 0);
        pz_frac = 0;
    }
    if (!any) return 0;
    long long ex = 0;
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < n && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; ++i; }
        const int e0 = i;
        for (; i < n; ++i) {
            const unsigned d = (unsigned)(unsigned char)s[i] - '0';
            if (d > 9u) break;
            if (ex < 1000000000ll) ex = ex * 10 + (long long)d;
        }
        if (i == e0) return 0;
        if (eneg) ex = -ex;
    }
    if (i != n) return 0;
    uint64_t bits = 0;
    if (w != 0) {
        if (many) return 0;
        q += ex + (long long)(pz - pz_frac);                              // trailing zeros before the point raise the exponent
        if (q < -DC_MAX_EXP10 || q > DC_MAX_EXP10) return 0;
        bits = dc_scale(w, (int)q);
    }
    if (neg) bits |= 1ull << 63;
    __builtin_memcpy(out, &bits, 8);
    return 1;
}
