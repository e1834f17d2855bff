// binary64 -> shortest decimal that reads back to the same double, in the layout of CPython's float.__repr__ (host
// and device).  The mirror of el_double.h: the writer of the pose JSON (jsonwrite.hip) prints with it what the parser
// reads with that one.
//
// Digits: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020; the steps of the 64-bit case are
// arranged as in A. Bolz's published C++ rendering of the paper, Drachennest).  The double's rounding interval, scaled by a power of
// ten from fmt_pow5_table.h so that its integer part holds the candidate digits, is computed with two 64 x 64 -> 128
// products per boundary, rounded to odd; the shortest decimal inside the interval wins, the one closest to the value
// among those of equal length, an exact tie going to the even digit.  That is what Ryu and Grisu-exact produce and what
// repr prints.  Integer arithmetic on the bit pattern only -- there is no `double` operation in this file, so host and
// device cannot differ by rounding or contraction -- and no decline path: every finite value gets its token.
//
// Layout (float_repr_style 'short', format code 'r'): with the digits d1 d2 .. dn and the decimal point in front of
// digit decpt + 1, positional for -4 < decpt <= 16 ("0.0001", "3.0", "1234.5", "1000000000000000.0"), otherwise
// d1[.d2..dn]e+XX / e-XX with at least two exponent digits ("1e-05", "1e+16", "5e-324"); "-0.0" for negative zero.  At
// most MPE_FMT_MAX_LEN = 24 bytes ("-1.2345678901234567e-308").
// tests/test_write_host.py holds the host build to repr under sanitizers, tests/test_gpu_write.py the device build.
#pragma once
#include <stdint.h>

#include "el_double.h"               // MPE_HD, el_mul64
#include "fmt_pow5_table.h"

#define MPE_FMT_MAX_LEN 24

namespace mpe {

#if defined(__HIP_DEVICE_COMPILE__)
__device__ static const uint64_t fmt_pow5[] = MPE_FMT_POW5_TABLE;
#else
static const uint64_t fmt_pow5[] = MPE_FMT_POW5_TABLE;
#endif

// floor(e * log2(10)), |e| <= 1233; floor(e * log10(2)) and floor(e * log10(2) + log10(3/4)), |e| <= 1500 (arithmetic shifts)
MPE_HD inline int fmt_floor_log2_pow10(int e) { return (e * 1741647) >> 19; }
MPE_HD inline int fmt_floor_log10_pow2(int e) { return (e * 1262611) >> 22; }
MPE_HD inline int fmt_floor_log10_three_quarters_pow2(int e) { return (e * 1262611 - 524031) >> 22; }

// cp * g / 2^128 for the 128-bit g = {ghi, glo}, rounded to odd: the last bit says "something was cut off"
MPE_HD inline uint64_t fmt_round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    uint64_t xhi, xlo, yhi, ylo;
    el_mul64(glo, cp, &xhi, &xlo);
    el_mul64(ghi, cp, &yhi, &ylo);
    const uint64_t y0 = ylo + xhi;
    const uint64_t y1 = yhi + (y0 < ylo ? 1u : 0u);
    return y1 | (y0 > 1 ? 1u : 0u);
}

// the finite, non-zero double with the biased exponent be and the fraction bits frac -> *digits * 10^*exp10, the
// shortest (*digits may still end in zeros when the value is an integer below 2^53)
MPE_HD inline void fmt_shortest(uint64_t frac, int be, uint64_t *digits, int *exp10) {
    uint64_t c;
    int q;
    if (be != 0) {
        c = ((uint64_t)1 << 52) | frac;
        q = be - 1075;
        if (0 <= -q && -q < 53 && (c & (((uint64_t)1 << -q) - 1)) == 0) {      // an integer: its own digits
            *digits = c >> -q;
            *exp10 = 0;
            return;
        }
    } else {
        c = frac;
        q = 1 - 1075;
    }
    const bool even = (c & 1) == 0;                      // the interval's ends belong to it when the significand is even
    const bool lower_closer = frac == 0 && be > 1;       // a power of two: the double below is half as far away
    const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0);
    const uint64_t cb = 4 * c;
    const uint64_t cbr = 4 * c + 2;
    const int k = lower_closer ? fmt_floor_log10_three_quarters_pow2(q) : fmt_floor_log10_pow2(q);
    const int h = q + fmt_floor_log2_pow10(-k) + 1;      // 1 .. 4
    const int idx = 2 * (-k - MPE_FMT_KMIN);
    const uint64_t ghi = fmt_pow5[idx], glo = fmt_pow5[idx + 1];
    const uint64_t vbl = fmt_round_to_odd(ghi, glo, cbl << h);
    const uint64_t vb = fmt_round_to_odd(ghi, glo, cb << h);
    const uint64_t vbr = fmt_round_to_odd(ghi, glo, cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1);
    const uint64_t upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb / 4;
    if (s >= 10) {                                       // one digit fewer: a multiple of ten inside the interval
        const uint64_t sp = s / 10;
        const bool up_inside = lower <= 40 * sp;
        const bool wp_inside = 40 * sp + 40 <= upper;
        if (up_inside != wp_inside) {
            *digits = sp + (wp_inside ? 1 : 0);
            *exp10 = k + 1;
            return;
        }
    }
    const bool u_inside = lower <= 4 * s;
    const bool w_inside = 4 * s + 4 <= upper;
    if (u_inside != w_inside) {
        *digits = s + (w_inside ? 1 : 0);
        *exp10 = k;
        return;
    }
    const uint64_t mid = 4 * s + 2;                      // both or neither: the closer one, a tie to the even digit
    const bool round_up = vb > mid || (vb == mid && (s & 1) != 0);
    *digits = s + (round_up ? 1 : 0);
    *exp10 = k;
}

// The token of the double with the bit pattern `bits` -> out[0 .. n), n <= MPE_FMT_MAX_LEN; returns n, 0 for an
// infinity or a NaN (JSON has no token for them; nothing is written).
MPE_HD inline int fmt_double(uint64_t bits, char *out) {
    const int be = (int)((bits >> 52) & 0x7FF);
    const uint64_t frac = bits & (((uint64_t)1 << 52) - 1);
    if (be == 0x7FF) return 0;
    int n = 0;
    if (bits >> 63) out[n++] = '-';
    if (be == 0 && frac == 0) {
        out[n++] = '0';
        out[n++] = '.';
        out[n++] = '0';
        return n;
    }
    uint64_t d;
    int e10;
    fmt_shortest(frac, be, &d, &e10);
    while (d % 10 == 0) {                                // d != 0
        d /= 10;
        ++e10;
    }
    int nd = 0;
    for (uint64_t t = d; t; t /= 10) ++nd;               // 1 .. 17
    const int decpt = nd + e10;
    if (decpt > -4 && decpt <= 16) {
        // positional; the digits are written from the last one backwards into their final places
        int first, point;                                // first digit's place, the point's place (-1: behind the digits)
        int end;
        if (decpt <= 0) {
            out[n] = '0';
            out[n + 1] = '.';
            for (int i = 0; i < -decpt; ++i) out[n + 2 + i] = '0';
            first = n + 2 - decpt;
            point = -1;
            end = first + nd;
        } else if (decpt < nd) {
            first = n;
            point = n + decpt;
            end = n + nd + 1;
        } else {
            first = n;
            point = -1;
            for (int i = nd; i < decpt; ++i) out[n + i] = '0';
            out[n + decpt] = '.';
            out[n + decpt + 1] = '0';
            end = n + decpt + 2;
        }
        int at = first + nd + (point >= 0 ? 1 : 0);
        for (int i = 0; i < nd; ++i) {
            --at;
            if (at == point) out[at--] = '.';
            out[at] = (char)('0' + (int)(d % 10));
            d /= 10;
        }
        return end;
    }
    // d1[.d2..dn]e+XX
    const int len = nd > 1 ? nd + 1 : 1;
    int at = n + len;
    for (int i = 0; i < nd - 1; ++i) {
        out[--at] = (char)('0' + (int)(d % 10));
        d /= 10;
    }
    if (nd > 1) out[--at] = '.';
    out[n] = (char)('0' + (int)d);
    n += len;
    int ex = decpt - 1;
    out[n++] = 'e';
    out[n++] = ex < 0 ? '-' : '+';
    if (ex < 0) ex = -ex;
    if (ex >= 100) {
        out[n++] = (char)('0' + ex / 100);
        ex %= 100;
    }
    out[n++] = (char)('0' + ex / 10);
    out[n++] = (char)('0' + ex % 10);
    return n;
}

// an integer as json.dumps writes it -> out[0 .. n), n <= 20
MPE_HD inline int fmt_int64(int64_t v, char *out) {
    int n = 0;
    uint64_t u = (uint64_t)v;
    if (v < 0) {
        out[n++] = '-';
        u = 0 - u;
    }
    int nd = 1;
    for (uint64_t t = u; t >= 10; t /= 10) ++nd;
    for (int i = nd - 1; i >= 0; --i) {
        out[n + i] = (char)('0' + (int)(u % 10));
        u /= 10;
    }
    return n + nd;
}

MPE_HD inline int fmt_int64_len(int64_t v) {
    uint64_t u = (uint64_t)v;
    int n = 1;
    if (v < 0) {
        u = 0 - u;
        ++n;
    }
    for (; u >= 10; u /= 10) ++n;
    return n;
}

}  // namespace mpe
