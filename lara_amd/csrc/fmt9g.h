// fmt9g.h -- "%.9g" of an fp32 value and the decimal text of a uint32, exactly, in integer arithmetic only; the same code on the
// host (plain C++) and on the device (hipcc).  lara_fmt9g(v) is C's / Python's "%.9g" % (double)v for every one of the 2^32 bit
// patterns (tools/meshio_exhaustive.cpp runs them all): nine significant digits correctly rounded from the exact binary value, ties
// to even; trailing zeros stripped; fixed notation when the decimal exponent X AFTER rounding satisfies -4 <= X < 9, otherwise
// d.ddde+XX; "-0" for negative zero; "nan" for every NaN whatever its sign; "inf" / "-inf".  The longest token has 15 characters.
//
// Method.  v = m 2^e with m < 2^24, -149 <= e <= 104.  The result is (q, k): q the nine digits, 10^8 <= q < 10^9, k the decimal
// exponent of the first one.
//   e < 0   k0 = floor((bitlength(v) - 1) log10 2) is k or k - 1.  N = m 10^(8 - k0) is an integer below 2^183 (v 10^(8 - k0) < 10^10
//           and e >= -149; 8 - k0 <= 53), held in six 32-bit limbs; w = N >> -e lies in [10^8, 10^10) and the bits shifted out say
//           whether the rest is below, at or above one half.  With w >= 10^9 the exponent was k0 + 1: q = w / 10, and the digit taken
//           off joins the rest.
//   e >= 0  the integer m 2^e < 2^128.  Below 10^9 it has nine digits or fewer and is exact.  Otherwise it is taken apart in base
//           10^9 (at most five chunks): the two leading chunks hold the nine digits and the digits that decide the rounding, every
//           chunk below them only whether the rest is zero.
// A carry out of the ninth digit (999999999.6 -> 1e+09) moves q back to 10^8 and k up by one before the notation is chosen.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LARA_FMT_HD __host__ __device__ __forceinline__
#else
#define LARA_FMT_HD inline
#endif

#define LARA_FMT9G_MAX_TOKEN 15    // e.g. -7.77995488e+32, -0.000123456789
#define LARA_FMT9G_LIMBS 6
#define LARA_FMT_U32_MAX_TOKEN 10

enum { LARA_DEC_FINITE = 0, LARA_DEC_ZERO = 1, LARA_DEC_INF = 2, LARA_DEC_NAN = 3 };

// the decimal form of one fp32 value: q nine digits of which the first nd are written, k the exponent of the first digit
struct lara_dec9 {
    uint32_t q;
    int32_t k;
    int32_t nd;
    uint32_t neg;
    uint32_t kind;
};

LARA_FMT_HD uint32_t lara_fmt_pow10(int n) {      // 10^n, 0 <= n <= 9
    uint32_t p = 1;
    for (int i = 0; i < n; ++i) p *= 10u;
    return p;
}

LARA_FMT_HD int lara_fmt_digits_u32(uint32_t v) {      // the number of decimal digits of v (1 for 0)
    int n = 1;
    for (uint32_t p = 10u; n < 10 && v >= p; p *= 10u) ++n;      // (10^10 does not fit: n stops at 10)
    return n;
}

LARA_FMT_HD lara_dec9 lara_fmt9g_decompose(float v) {
    uint32_t bits;
    __builtin_memcpy(&bits, &v, 4);
    lara_dec9 d;
    d.q = 0, d.k = 0, d.nd = 1, d.neg = bits >> 31, d.kind = LARA_DEC_FINITE;
    const uint32_t ex = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
    if (ex == 255u) {
        d.kind = frac ? LARA_DEC_NAN : LARA_DEC_INF;
        return d;
    }
    if ((ex | frac) == 0u) {
        d.kind = LARA_DEC_ZERO;
        return d;
    }
    const uint32_t m = ex ? (frac | 0x800000u) : frac;
    const int e = ex ? (int)ex - 150 : -149;
    uint32_t q;
    int k;
    int up = 0, tie = 0;      // the rest is above one half / exactly one half
    if (e < 0) {
        const int s = -e;                                                  // 1 .. 149
        const int top = 31 - __builtin_clz(m) + e;                         // 2^top <= v < 2^(top + 1)
        const int k0 = (top * 1233) >> 12;                                 // floor(top log10 2) for |top| < 200: k or k - 1
        const int p = 8 - k0;                                              // 0 <= p <= 53 (v < 2^24)
        uint32_t L[LARA_FMT9G_LIMBS];
        L[0] = m;
        for (int i = 1; i < LARA_FMT9G_LIMBS; ++i) L[i] = 0u;
        for (int step = 0; step <= p / 9; ++step) {                        // p / 9 factors of 10^9, then 10^(p % 9)
            const uint32_t f = step < p / 9 ? 1000000000u : lara_fmt_pow10(p % 9);
            uint64_t carry = 0;
            for (int i = 0; i < LARA_FMT9G_LIMBS; ++i) {
                const uint64_t t = (uint64_t)L[i] * f + carry;
                L[i] = (uint32_t)t;
                carry = t >> 32;
            }
#ifdef LARA_FMT9G_CHECK
            if (carry) LARA_FMT9G_CHECK;
#endif
        }
        // w = N >> s (34 bits at the most), the bit below it, and whether anything lies below that
        const int i0 = s >> 5, sh = s & 31, h = s - 1, ih = h >> 5;
        uint32_t a0 = 0, a1 = 0, a2 = 0, below = 0, half = 0;
        for (int i = 0; i < LARA_FMT9G_LIMBS; ++i) {
            if (i == i0) a0 = L[i];
            if (i == i0 + 1) a1 = L[i];
            if (i == i0 + 2) a2 = L[i];
            if (i < ih) below |= L[i];
            if (i == ih) {
                half = (L[i] >> (h & 31)) & 1u;
                below |= L[i] & ((1u << (h & 31)) - 1u);
            }
        }
        const uint64_t lo = (uint64_t)a0 | ((uint64_t)a1 << 32);
        const uint64_t w = sh ? (lo >> sh) | ((uint64_t)a2 << (64 - sh)) : lo;
        if (w >= 1000000000ull) {
            const uint32_t r = (uint32_t)(w % 10ull);
            const int rest = (half | below) != 0u;
            q = (uint32_t)(w / 10ull);
            k = k0 + 1;
            up = r > 5u || (r == 5u && rest);
            tie = r == 5u && !rest;
        } else {
            q = (uint32_t)w;
            k = k0;
            up = half && below;
            tie = half && !below;
        }
    } else if (e <= 6 && (m << e) < 1000000000u) {
        const uint32_t n = m << e;
        k = lara_fmt_digits_u32(n) - 1;
        q = n * lara_fmt_pow10(8 - k);
    } else {
        uint32_t L[4] = {0u, 0u, 0u, 0u};
        const uint64_t x = (uint64_t)m << (e & 31);
        for (int i = 0; i < 4; ++i) {
            if (i == (e >> 5)) L[i] = (uint32_t)x;
            if (i == (e >> 5) + 1) L[i] = (uint32_t)(x >> 32);
        }
        uint32_t hi = 0, lo = 0, sticky = 0;
        int n = 0;
        for (int j = 0; j < 5; ++j) {
            if ((L[0] | L[1] | L[2] | L[3]) == 0u) break;
            uint64_t rem = 0;
            for (int i = 3; i >= 0; --i) {
                const uint64_t cur = (rem << 32) | L[i];
                L[i] = (uint32_t)(cur / 1000000000ull);
                rem = cur % 1000000000ull;
            }
            sticky |= lo;
            lo = hi;
            hi = (uint32_t)rem;
            ++n;
        }
        const int dg = lara_fmt_digits_u32(hi);                            // hi != 0; n >= 2 since v >= 10^9
        k = 9 * (n - 1) + dg - 1;
        uint32_t r, mid;
        if (dg == 9) {
            q = hi, r = lo, mid = 500000000u;
        } else {
            const uint32_t pw = lara_fmt_pow10(dg);
            q = hi * lara_fmt_pow10(9 - dg) + lo / pw;
            r = lo % pw;
            mid = pw / 2u;
        }
        up = r > mid || (r == mid && sticky);
        tie = r == mid && !sticky;
    }
    if (up || (tie && (q & 1u))) ++q;
    if (q == 1000000000u) q = 100000000u, ++k;
    int nd = 9;
    for (uint32_t t = q; nd > 1 && t % 10u == 0u; t /= 10u) --nd;
    d.q = q, d.k = k, d.nd = nd;
    return d;
}

LARA_FMT_HD int lara_fmt9g_len(const lara_dec9 d) {
    if (d.kind == LARA_DEC_ZERO) return 1 + (int)d.neg;
    if (d.kind == LARA_DEC_INF) return 3 + (int)d.neg;
    if (d.kind == LARA_DEC_NAN) return 3;
    int n;
    if (d.k >= 9 || d.k < -4)
        n = (d.nd > 1 ? 1 + d.nd : 1) + 4;
    else if (d.k >= 0)
        n = d.k + 1 + (d.nd > d.k + 1 ? d.nd - d.k : 0);
    else
        n = 1 - d.k + d.nd;
    return n + (int)d.neg;
}

// writes the token (no terminator, nothing beyond its length) and returns its length
template <class Char>
LARA_FMT_HD int lara_fmt9g_write(const lara_dec9 d, Char *out) {
    int o = 0;
    if (d.neg && d.kind != LARA_DEC_NAN) out[o++] = '-';
    if (d.kind == LARA_DEC_ZERO) {
        out[o++] = '0';
        return o;
    }
    if (d.kind == LARA_DEC_INF) {
        out[o] = 'i', out[o + 1] = 'n', out[o + 2] = 'f';
        return o + 3;
    }
    if (d.kind == LARA_DEC_NAN) {
        out[o] = 'n', out[o + 1] = 'a', out[o + 2] = 'n';
        return o + 3;
    }
    const int sci = d.k >= 9 || d.k < -4;
    const int whole = (sci || d.k < 0) ? 0 : d.k;          // digits 0 .. whole stand in front of the point
    const int lead = (!sci && d.k < 0) ? 1 - d.k : 0;      // "0." and -k - 1 zeros in front of the first digit
    if (lead) {
        out[o] = '0', out[o + 1] = '.';
        for (int i = 2; i < lead; ++i) out[o + i] = '0';
        o += lead;
    }
    uint32_t t = d.q;
    for (int i = 8; i >= 0; --i) {
        const char c = (char)('0' + t % 10u);
        t /= 10u;
        if (i <= whole)
            out[o + i] = c;
        else if (i < d.nd)
            out[o + i + (lead ? 0 : 1)] = c;
    }
    if (!lead && d.nd > whole + 1) out[o + whole + 1] = '.';
    o += lead ? d.nd : (d.nd > whole + 1 ? d.nd + 1 : whole + 1);
    if (sci) {
        const int a = d.k < 0 ? -d.k : d.k;                // at most 45: always two digits
        out[o] = 'e', out[o + 1] = d.k < 0 ? '-' : '+', out[o + 2] = (char)('0' + a / 10), out[o + 3] = (char)('0' + a % 10);
        o += 4;
    }
    return o;
}

LARA_FMT_HD int lara_fmt9g(float v, char out[16]) { return lara_fmt9g_write(lara_fmt9g_decompose(v), out); }

template <class Char>
LARA_FMT_HD int lara_fmt_u32_write(uint32_t v, Char *out) {
    const int n = lara_fmt_digits_u32(v);
    for (int i = n - 1; i >= 0; --i) {
        out[i] = (char)('0' + v % 10u);
        v /= 10u;
    }
    return n;
}

LARA_FMT_HD int lara_fmt_u32(uint32_t v, char out[10]) { return lara_fmt_u32_write(v, out); }
