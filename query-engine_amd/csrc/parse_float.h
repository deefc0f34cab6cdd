// Text of one CSV cell to its value (k_csv.hip), the inverse of fmt_float.h: host and device from
// one source (`__device__` is defined away for the host build, tests/parse_host.cpp).
//
// Float64: the correctly rounded double of a decimal (round half to even, overflow to +-inf,
// subnormals, -0.0) -- Python's float(cell) bit for bit -- or the answer "cannot decide":
//   * W. Clinger's exact fast path ("How to read floating point numbers accurately", 1990): at most
//     53 significant bits times or divided by 10^|q|, |q| <= 22, is one correctly rounded operation
//     on two exact doubles;
//   * Eisel-Lemire (D. Lemire, "Number parsing at a gigabyte per second", 2021): the 64-bit decimal
//     significand times a 128-bit truncated power of five (tools/gen_lemire_table.py), rounded from
//     the product's top bits;
//   * kParseUndecided for everything else: the product's low bits all ones outside the proven
//     exponent range, and more than 19 significant digits whose truncated and incremented
//     significands round to different doubles.  The caller parses those cells on the host.
// Every reader takes the cell through `Src::at(i)` (absolute byte index) so that the kernel can read
// through its word cache and the host from a plain buffer.
#pragma once

#include <cstdint>

#include "parse_float_table.h"

namespace qeh {

enum { kParseOk = 0, kParseUndecided = 1, kParseBad = 2 };

__device__ const double kPfExact10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                          1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

constexpr uint64_t kPfInf = 0x7FF0000000000000ull;

// w * 10^q, w != 0, to the bits of the nearest double (no sign)
__device__ inline int pf_eisel_lemire(uint64_t w, int64_t q, uint64_t *bits) {
    if (q < kPfQMin) {  // w < 2^64 < 1.9e19: below half the smallest subnormal
        *bits = 0;
        return kParseOk;
    }
    if (q > kPfQMax) {
        *bits = kPfInf;
        return kParseOk;
    }
    int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t ph = kPfPow5[2 * (q - kPfQMin)], pl = kPfPow5[2 * (q - kPfQMin) + 1];
    const unsigned __int128 first = (unsigned __int128)w * ph;
    uint64_t lo = (uint64_t)first, hi = (uint64_t)(first >> 64);
    if ((hi & 0x1FFu) == 0x1FFu) {  // the 55 bits that matter may still change: add the low half
        const uint64_t sh = (uint64_t)(((unsigned __int128)w * pl) >> 64);
        lo += sh;
        if (sh > lo) ++hi;
    }
    if (lo == ~0ull && (q < -27 || q > 55)) return kParseUndecided;
    const int upperbit = (int)(hi >> 63);
    uint64_t m = hi >> (upperbit + 9);  // 52 + 3 bits
    int64_t power2 = ((217706 * q) >> 16) + 63 + upperbit - lz + 1023;  // biased exponent
    if (power2 <= 0) {                                                  // subnormal (or the smallest normal)
        if (-power2 + 1 >= 64) {
            *bits = 0;
            return kParseOk;
        }
        m >>= -power2 + 1;
        m += m & 1;
        m >>= 1;
        *bits = m;  // m = 2^52 is the smallest normal: its bit 52 is the exponent 1
        return kParseOk;
    }
    // exactly halfway between two doubles (only possible when 5^q fits 64 bits): ties to even
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << (upperbit + 9)) == hi) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) {
        m = 1ull << 52;
        ++power2;
    }
    m &= ~(1ull << 52);
    if (power2 >= 0x7FF) {
        *bits = kPfInf;
        return kParseOk;
    }
    *bits = m | ((uint64_t)power2 << 52);
    return kParseOk;
}

// (-1)^neg * w * 10^q; `truncated`: digits beyond w's 19 were dropped, the value lies in (w, w + 1) * 10^q
__device__ inline int pf_decimal(bool neg, uint64_t w, int64_t q, bool truncated, uint64_t *bits) {
    uint64_t r = 0;
    if (w == 0) {
        r = 0;
    } else if (!truncated && w <= (1ull << 53) && q >= -22 && q <= 22) {
        double d = (double)w;
        d = q < 0 ? d / kPfExact10[-q] : d * kPfExact10[q];
        __builtin_memcpy(&r, &d, 8);
    } else {
        int s = pf_eisel_lemire(w, q, &r);
        if (s != kParseOk) return s;
        if (truncated) {
            uint64_t r2 = 0;
            s = pf_eisel_lemire(w + 1, q, &r2);
            if (s != kParseOk || r2 != r) return kParseUndecided;
        }
    }
    *bits = r | ((uint64_t)neg << 63);
    return kParseOk;
}

__device__ inline bool pf_digit(uint8_t c) { return (uint8_t)(c - '0') < 10u; }

// ASCII case-insensitive match of s[a, b) with the lower-case word `word` of length n
template <class Src>
__device__ inline bool pf_word(Src &s, int64_t a, int64_t b, const char *word, int n) {
    if (b - a != n) return false;
    for (int i = 0; i < n; ++i)
        if ((s.at(a + i) | 0x20) != (uint8_t)word[i]) return false;
    return true;
}

// -?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)? or nan / inf / infinity with an optional '-'
template <class Src>
__device__ inline int parse_f64_text(Src &s, int64_t a, int64_t b, uint64_t *bits) {
    bool neg = false;
    if (a < b && s.at(a) == '-') neg = true, ++a;
    if (a >= b) return kParseBad;
    const uint8_t c0 = s.at(a);
    if (!pf_digit(c0) && c0 != '.') {
        uint64_t r;
        if (pf_word(s, a, b, "nan", 3)) r = 0x7FF8000000000000ull;
        else if (pf_word(s, a, b, "inf", 3) || pf_word(s, a, b, "infinity", 8)) r = kPfInf;
        else return kParseBad;
        *bits = r | ((uint64_t)neg << 63);
        return kParseOk;
    }
    uint64_t w = 0;
    int nd = 0;       // significant digits in w (<= 19)
    int64_t q = 0;    // the value is w * 10^q (plus the dropped digits)
    bool truncated = false, any = false, frac = false;
    int64_t i = a;
    for (; i < b; ++i) {
        const uint8_t c = s.at(i);
        if (c == '.') {
            if (frac) return kParseBad;
            frac = true;
            continue;
        }
        if (!pf_digit(c)) break;
        any = true;
        const uint32_t d = (uint32_t)(c - '0');
        if (nd < 19) {
            if (w != 0 || d != 0) w = w * 10 + d, ++nd;
            if (frac) --q;
        } else {
            if (d != 0) truncated = true;
            if (!frac) ++q;
        }
    }
    if (!any) return kParseBad;
    if (i < b) {
        if ((s.at(i) | 0x20) != 'e') return kParseBad;
        ++i;
        bool eneg = false;
        if (i < b && (s.at(i) == '+' || s.at(i) == '-')) eneg = s.at(i) == '-', ++i;
        if (i >= b) return kParseBad;
        int64_t e = 0;
        for (; i < b; ++i) {
            const uint8_t c = s.at(i);
            if (!pf_digit(c)) return kParseBad;
            if (e < 100000000) e = e * 10 + (c - '0');  // (saturates far outside the double range)
        }
        q += eneg ? -e : e;
    }
    if (q < -1000000) q = -1000000;
    if (q > 1000000) q = 1000000;
    return pf_decimal(neg, w, q, truncated, bits);
}

// -?[0-9]+ within [-(max + 1), max]
template <class Src>
__device__ inline int parse_int_text(Src &s, int64_t a, int64_t b, uint64_t max, int64_t *out) {
    bool neg = false;
    if (a < b && s.at(a) == '-') neg = true, ++a;
    if (a >= b) return kParseBad;
    const uint64_t lim = max + (neg ? 1u : 0u);
    uint64_t v = 0;
    for (int64_t i = a; i < b; ++i) {
        const uint8_t c = s.at(i);
        if (!pf_digit(c)) return kParseBad;
        const uint64_t d = (uint64_t)(c - '0');
        if (v > (lim - d) / 10) return kParseBad;  // v * 10 + d > lim
        v = v * 10 + d;
    }
    *out = neg ? (int64_t)(0 - v) : (int64_t)v;
    return kParseOk;
}

template <class Src>
__device__ inline int parse_bool_text(Src &s, int64_t a, int64_t b, bool *out) {
    if (pf_word(s, a, b, "true", 4)) *out = true;
    else if (pf_word(s, a, b, "false", 5)) *out = false;
    else return kParseBad;
    return kParseOk;
}

// YYYY-MM-DD, a proleptic-Gregorian date of the years 0001-9999, as days since 1970-01-01
template <class Src>
__device__ inline int parse_date32_text(Src &s, int64_t a, int64_t b, int32_t *out) {
    if (b - a != 10) return kParseBad;
    uint32_t v[3] = {0, 0, 0};
    for (int i = 0; i < 10; ++i) {
        const uint8_t c = s.at(a + i);
        if (i == 4 || i == 7) {
            if (c != '-') return kParseBad;
        } else {
            if (!pf_digit(c)) return kParseBad;
            const int k = i < 4 ? 0 : i < 7 ? 1 : 2;
            v[k] = v[k] * 10 + (uint32_t)(c - '0');
        }
    }
    const uint32_t y = v[0], m = v[1], d = v[2];
    if (y < 1 || m < 1 || m > 12 || d < 1) return kParseBad;
    const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
    const uint32_t dim = m == 2 ? (leap ? 29u : 28u) : (m == 4 || m == 6 || m == 9 || m == 11) ? 30u : 31u;
    if (d > dim) return kParseBad;
    // days from civil, the year counted from March (the inverse of k_encode.hip's put_date)
    const uint32_t yy = m <= 2 ? y - 1 : y;
    const uint32_t era = yy / 400, yoe = yy - era * 400;
    const uint32_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
    const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    *out = (int32_t)(era * 146097 + doe) - 719468;
    return kParseOk;
}

}  // namespace qeh
