// bed_fmt.h — the text of `wgbstools beta2bed`'s columns, one rule for host and device: decimal digits of an integer, and awk's
// printf "%.3g" of the double meth / cov (beta2bed.py:18) from the two counts alone, byte for byte, ties included.
// Below it, by the same argument, printf "%.3f" of that double for `wgbstools beta_to_450k` (wg_fmt_f3).
// No HIP needed: g++ compiles it alone (tests/native/bed_host.cpp and array_host.cpp are the CPU suite's twins of what the kernels run).
//
// "%.3g" prints the EXACT value of the double v = fl(m / c), rounded to three significant decimal digits, half to even.  v differs
// from the rational m / c by less than one ulp, so the three digits come from the integers: q, r = divmod(m * 10^(2 - e), c) with
// e = floor(log10(m / c)); r decides the rounding unless 2 r == den, the exact rational tie.  There the double lies on the tie
// or an ulp's fraction beside it, and the side is the sign of fma(v, c, -m) = v * c - m, which fp64 holds exactly (v * c needs
// at most 53 + 16 bits, the difference is below one ulp of m).  Zero: v is the tie itself, half to even on q.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef WG_HD                          // (exact_log2.h has the same two lines)
#if defined(__HIPCC__)
#define WG_HD __host__ __device__ __forceinline__
#else
#define WG_HD static inline
#endif
#endif

#define WG_G3_MAX_LEN 8                // "0.000123", "1.53e-05", "6.55e+04"

// decimal digits of v (1 for 0)
WG_HD int wg_dec_len(uint64_t v)
{
    int n = 1;
    while (v >= 10) { v /= 10; n++; }
    return n;
}

// the decimal digits of v at dst (its wg_dec_len(v) bytes); -> their number
template <class P>
WG_HD int wg_dec_put(P dst, uint64_t v)
{
    const int n = wg_dec_len(v);
    for (int i = n - 1; i >= 0; i--) { dst[i] = (char)('0' + (int)(v % 10)); v /= 10; }
    return n;
}

WG_HD uint64_t wg_p10(int k)
{
    uint64_t p = 1;
    for (int i = 0; i < k; i++) p *= 10;
    return p;
}

// digit i (0: hundreds) of q = 100 .. 999
WG_HD uint32_t wg_g3_digit(uint32_t q, int i) { return i == 0 ? q / 100 : i == 1 ? q / 10 % 10 : q % 10; }

// "%.3g" of the double m / c for counts m >= 0, c > 0 below 2^16: the text's bytes packed into the result, first character in
// the lowest byte, *len of them (at most WG_G3_MAX_LEN).  m > c is a value like any other.
WG_HD uint64_t wg_fmt_g3(uint32_t m, uint32_t c, int* len)
{
    if (m == 0) { *len = 1; return (uint64_t)'0'; }
    // e = floor(log10(m / c)): the largest e with c * 10^e <= m; -5 .. 4 for 16-bit counts
    int e = 4;
    for (; e > -5; e--) {
        const bool ge = e >= 0 ? (uint64_t)m >= (uint64_t)c * wg_p10(e) : (uint64_t)m * wg_p10(-e) >= (uint64_t)c;
        if (ge) break;
    }
    const uint64_t num = e <= 2 ? (uint64_t)m * wg_p10(2 - e) : (uint64_t)m;
    const uint64_t den = e <= 2 ? (uint64_t)c : (uint64_t)c * wg_p10(e - 2);
    uint32_t q = (uint32_t)(num / den);                          // 100 .. 999
    const uint64_t r2 = 2 * (num % den);
    bool up = r2 > den;
    if (r2 == den) {
        const double v = (double)m / (double)c;
        const double s = fma(v, (double)c, -(double)m);
        up = s > 0.0 || (s == 0.0 && (q & 1u));
    }
    if (up) q++;
    if (q == 1000) { q = 100; e++; }
    const int nd = q % 10 ? 3 : q % 100 ? 2 : 1;                    // significant digits left once trailing zeros go
    uint64_t out = 0;
    int n = 0;
#define WG_G3_PUT(ch) (out |= (uint64_t)(uint8_t)(ch) << (8 * n), n++)
    if (e < -4 || e >= 3) {                                      // d[.dd]e+XX
        WG_G3_PUT('0' + wg_g3_digit(q, 0));
        if (nd > 1) {
            WG_G3_PUT('.');
            for (int i = 1; i < nd; i++) WG_G3_PUT('0' + wg_g3_digit(q, i));
        }
        const int ae = e < 0 ? -e : e;
        WG_G3_PUT('e');
        WG_G3_PUT(e < 0 ? '-' : '+');
        WG_G3_PUT('0' + ae / 10);
        WG_G3_PUT('0' + ae % 10);
    } else if (e >= 0) {                                         // e + 1 digits, then what is left of the three
        for (int i = 0; i <= e; i++) WG_G3_PUT('0' + wg_g3_digit(q, i));
        if (nd > e + 1) {
            WG_G3_PUT('.');
            for (int i = e + 1; i < nd; i++) WG_G3_PUT('0' + wg_g3_digit(q, i));
        }
    } else {                                                     // 0.[zeros]ddd
        WG_G3_PUT('0');
        WG_G3_PUT('.');
        for (int i = 0; i < -e - 1; i++) WG_G3_PUT('0');
        for (int i = 0; i < nd; i++) WG_G3_PUT('0' + wg_g3_digit(q, i));
    }
#undef WG_G3_PUT
    *len = n;
    return out;
}

// "%.3f" of the double m / c for counts m >= 0, c > 0 below 2^16 (`wgbstools beta_to_450k`): the value in thousandths, rounded as C
// rounds the EXACT value of v = fl(m / c), half to even.  q, r = divmod(1000 m, c); r decides unless 2 r == c, the exact rational tie,
// where — as in wg_fmt_g3 — the side is the sign of fma(v, c, -m) and zero goes half to even on q.  The text is q / 1000, a point and
// the three digits of q % 1000: wg_f3_len / wg_f3_put, at most WG_F3_MAX_LEN bytes.
#define WG_F3_MAX_LEN 9                // "65535.000"

WG_HD uint32_t wg_fmt_f3(uint32_t m, uint32_t c)
{
    const uint32_t num = 1000u * m;                              // below 2^26
    uint32_t q = num / c;
    const uint32_t r2 = 2u * (num - q * c);
    bool up = r2 > c;
    if (r2 == c) {
        const double v = (double)m / (double)c;
        const double s = fma(v, (double)c, -(double)m);
        up = s > 0.0 || (s == 0.0 && (q & 1u));
    }
    return up ? q + 1 : q;
}

WG_HD int wg_f3_len(uint32_t q) { return wg_dec_len(q / 1000u) + 4; }

// the text of q thousandths at dst (its wg_f3_len(q) bytes); -> their number
template <class P>
WG_HD int wg_f3_put(P dst, uint32_t q)
{
    const int n = wg_dec_put(dst, q / 1000u);
    const uint32_t f = q % 1000u;
    dst[n] = '.';
    dst[n + 1] = (char)('0' + f / 100u);
    dst[n + 2] = (char)('0' + f / 10u % 10u);
    dst[n + 3] = (char)('0' + f % 10u);
    return n + 4;
}
