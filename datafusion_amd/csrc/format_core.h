// CAST to Utf8 (DFMI_FLAG_EXT_CAST_UTF8, DESIGN.md §4 "CAST to Utf8"): the
// formatting core -- digit count, integer digits, shortest float digits and
// the positional layout -- as plain C++ with no library call and no wave
// intrinsic: one text for the device kernels (format.hip) and for the host
// driver that checks it against std::to_chars under ASan + UBSan
// (tests/native/format_driver.cpp), in the way avg_round.h is shared.
//
// A value is first reduced to a `Dec` (sign, up to 20 decimal digits, the
// position of the point), then laid out byte by byte: fmt_length() is what
// the measure pass writes, fmt_byte() what the write pass stores, so the two
// passes agree by construction and no row needs a 327-byte buffer.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DFMI_HD __host__ __device__
#else
#define DFMI_HD
#endif

namespace dfmi {
namespace fmt {

typedef unsigned long long u64;
typedef unsigned u32;

enum Kind : int { kNumber = 0, kInf = 1, kNaN = 2, kTrue = 3, kFalse = 4 };

// Which path gave a float's digits (the probe's statistics).
enum Path : int { kPathSpecial = 0, kPathInteger = 1, kPathDecimal = 2, kPathExact = 3 };

// value = (-1)^neg * 0.d0 d1 .. d(nd-1) * 10^pt; digit i is byte (i & 7) of p[i >> 3].
struct Dec {
    u64 p[3];
    int nd, pt, neg, kind;
};

DFMI_HD inline void dec_clear(Dec& d) {
    d.p[0] = d.p[1] = d.p[2] = 0;
    d.nd = 0, d.pt = 0, d.neg = 0, d.kind = kNumber;
}
DFMI_HD inline void dec_set(Dec& d, int i, u32 digit) {
    const u64 b = (u64)digit << ((i & 7) * 8);
    if (i < 8) d.p[0] |= b;
    else if (i < 16) d.p[1] |= b;
    else d.p[2] |= b;
}
DFMI_HD inline u32 dec_get(const Dec& d, int i) {
    const u64 w = i < 8 ? d.p[0] : (i < 16 ? d.p[1] : d.p[2]);
    return (u32)(w >> ((i & 7) * 8)) & 0xffu;
}

// Decimal digits of v (1 for zero): compares only, no division.
DFMI_HD inline int digits10_u32(u32 v) {
    if (v < 100u) return v < 10u ? 1 : 2;
    if (v < 10000u) return v < 1000u ? 3 : 4;
    if (v < 1000000u) return v < 100000u ? 5 : 6;
    if (v < 100000000u) return v < 10000000u ? 7 : 8;
    return v < 1000000000u ? 9 : 10;
}
DFMI_HD inline int digits10_u64(u64 v) {
    if (v < 4294967296ull) return digits10_u32((u32)v);
    if (v < 1000000000000ull) return v < 10000000000ull ? 10 : (v < 100000000000ull ? 11 : 12);
    if (v < 10000000000000000ull) {
        if (v < 100000000000000ull) return v < 10000000000000ull ? 13 : 14;
        return v < 1000000000000000ull ? 15 : 16;
    }
    if (v < 1000000000000000000ull) return v < 100000000000000000ull ? 17 : 18;
    return v < 10000000000000000000ull ? 19 : 20;
}

// The digits of the integer v: nd = its digit count, pt = nd (divisors are constants: multiply-high).
DFMI_HD inline void dec_from_u64(Dec& d, u64 v, int neg) {
    dec_clear(d);
    d.neg = neg;
    const int nd = digits10_u64(v);
    d.nd = d.pt = nd;
    int i = nd - 1;
    while (v >= 4294967296ull) {
        const u64 q = v / 10ull;
        dec_set(d, i--, (u32)(v - q * 10ull));
        v = q;
    }
    u32 w = (u32)v;
    for (; i >= 0; --i) {
        const u32 q = w / 10u;
        dec_set(d, i, w - q * 10u);
        w = q;
    }
}

// ---------------------------------------------------------------------------
// The exact shortest digits: free-format digit generation (Steele & White /
// Dragon4 in Burger & Dybvig's integer form) over 32-bit words.
//   v = m * 2^e = r / s, half the gap to the next float above = mp / s, below
//   = mm / s (mp = mm, or 2 mm at a power of two). Digits are produced while
//   the remainder could still be a different float's; the interval's ends
//   count as inside when m is even (they read back to v by ties-to-even).
// 36 words hold the largest operand: s = 2^1076 * 10^2 and r < 10 s for 5e-324.
constexpr int kBigWords = 36;
struct Big {
    u32 w[kBigWords];
    int n;  // words in use (an upper bound; the words above are zero)
};

DFMI_HD inline void big_zero(Big& a) {
    for (int i = 0; i < kBigWords; ++i) a.w[i] = 0;
    a.n = 1;
}
// a = m * 2^sh
DFMI_HD inline void big_set_shifted(Big& a, u64 m, int sh) {
    big_zero(a);
    const int word = sh >> 5, bit = sh & 31;
    a.w[word] = (u32)(m << bit);
    a.w[word + 1] = bit ? (u32)(m >> (32 - bit)) : (u32)(m >> 32);
    a.w[word + 2] = bit ? (u32)(m >> (64 - bit)) : 0u;
    a.n = word + 3;
}
DFMI_HD inline void big_mul_small(Big& a, u32 k) {
    u64 c = 0;
    for (int i = 0; i < a.n; ++i) {
        c += (u64)a.w[i] * k;
        a.w[i] = (u32)c;
        c >>= 32;
    }
    if (c && a.n < kBigWords) a.w[a.n++] = (u32)c;
}
DFMI_HD inline void big_mul_pow10(Big& a, int k) {
    for (; k >= 9; k -= 9) big_mul_small(a, 1000000000u);
    if (k > 0) {
        u32 p = 1;
        for (int i = 0; i < k; ++i) p *= 10u;
        big_mul_small(a, p);
    }
}
// sign of (r + c * m) - s over n words, c in {0, 1, 2}
DFMI_HD inline int big_cmp_sum(const Big& r, const Big& m, u32 c, const Big& s, int n) {
    u64 carry = 0;
    int res = 0;
    for (int i = 0; i < n; ++i) {
        const u64 t = (u64)r.w[i] + (u64)m.w[i] * c + carry;
        const u32 lo = (u32)t;
        carry = t >> 32;
        if (lo != s.w[i]) res = lo > s.w[i] ? 1 : -1;
    }
    return carry ? 1 : res;
}
// sign of 2 r - s
DFMI_HD inline int big_cmp_twice(const Big& r, const Big& s, int n) { return big_cmp_sum(r, r, 1, s, n); }
// sign of a - b
DFMI_HD inline int big_cmp(const Big& a, const Big& b, int n) {
    for (int i = n - 1; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i] ? 1 : -1;
    return 0;
}
// r -= s (r >= s)
DFMI_HD inline void big_sub(Big& r, const Big& s, int n) {
    u64 borrow = 0;
    for (int i = 0; i < n; ++i) {
        const u64 t = (u64)r.w[i] - s.w[i] - borrow;
        r.w[i] = (u32)t;
        borrow = (t >> 32) & 1u;
    }
}
DFMI_HD inline int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// v = m * 2^e > 0 (m < 2^53); `boundary`: the gap below v is half the gap above.
DFMI_HD inline void shortest_exact(Dec& d, u64 m, int e, bool boundary) {
    const bool even = (m & 1ull) == 0;
    Big r, s, mm;
    const u32 mpc = boundary ? 2u : 1u;  // mp = mpc * mm
    const int two = boundary ? 2 : 1;    // r and s carry a factor 2 (4 at a boundary)
    if (e >= 0) {
        big_set_shifted(r, m, e + two);
        big_set_shifted(s, 1ull, two);
        big_set_shifted(mm, 1ull, e);
    } else {
        big_set_shifted(r, m, two);
        big_set_shifted(s, 1ull, -e + two);
        big_set_shifted(mm, 1ull, 0);
    }
    // k0 <= floor(log10 v): b = floor(log2 v), log10(2) bracketed by 315652 / 2^20 < log10(2) < 315653 / 2^20
    int hb = 52;
    while (hb > 0 && !((m >> hb) & 1ull)) --hb;
    const int b = hb + e;
    int k = b >= 0 ? (int)(((long long)b * 315652ll) >> 20) : -(int)((((long long)-b) * 315653ll + 1048575ll) >> 20);
    if (k >= 0) big_mul_pow10(s, k);
    else {
        big_mul_pow10(r, -k);
        big_mul_pow10(mm, -k);
    }
    // the least k with (r + mp) / s < 1 (<= 1 where the end itself is excluded): v = 0.d0 d1 .. * 10^k
    for (;;) {
        const int n = max3(r.n, s.n, mm.n);
        const int c = big_cmp_sum(r, mm, mpc, s, n);
        if (!(even ? c >= 0 : c > 0)) break;
        big_mul_small(s, 10u);
        ++k;
    }
    d.pt = k;
    int nd = 0;
    for (;;) {
        big_mul_small(r, 10u);
        big_mul_small(mm, 10u);
        const int n = max3(r.n, s.n, mm.n);
        u32 digit = 0;
        while (big_cmp(r, s, n) >= 0) {
            big_sub(r, s, n);
            ++digit;
        }
        const int cl = big_cmp(r, mm, n);
        const bool low = even ? cl <= 0 : cl < 0;
        const int ch = big_cmp_sum(r, mm, mpc, s, n);
        const bool high = even ? ch >= 0 : ch > 0;
        if (!low && !high) {
            if (nd < 20) dec_set(d, nd, digit);
            ++nd;
            continue;
        }
        if (low && high) {  // both neighbours read back: the closer, a tie to the even digit
            const int c2 = big_cmp_twice(r, s, n);
            if (c2 > 0 || (c2 == 0 && (digit & 1u))) ++digit;
        } else if (high) {
            ++digit;
        }
        if (nd < 20) dec_set(d, nd, digit);
        ++nd;
        break;
    }
    d.nd = nd;
}

// Shortest digits of a float given by its bits. F32: a Float32 in the low 32 bits.
template <bool F32>
DFMI_HD inline int dec_from_float(Dec& d, u64 bits) {
    constexpr int P = F32 ? 23 : 52;         // fraction bits
    constexpr int EB = F32 ? 8 : 11;         // exponent bits
    constexpr int BIAS = F32 ? 127 : 1023;
    dec_clear(d);
    d.neg = (int)((bits >> (P + EB)) & 1ull);
    const u64 frac = bits & ((1ull << P) - 1);
    const int E = (int)((bits >> P) & ((1u << EB) - 1));
    if (E == (1 << EB) - 1) {
        d.kind = frac ? kNaN : kInf;
        if (frac) d.neg = 0;  // every NaN is "NaN"
        return kPathSpecial;
    }
    if (E == 0 && frac == 0) {  // "0" / "-0"
        d.nd = d.pt = 1;
        return kPathSpecial;
    }
    const u64 m = E ? (frac | (1ull << P)) : frac;
    const int e = (E ? E : 1) - BIAS - P;
    // (a) an integer below 2^(P+1): its own digits are the shortest -- a shorter string
    //     differs from it by at least 1, more than half the gap (at most 1/2)
    if (e >= 0 ? (E - BIAS <= P) : (-e <= P && (m & ((1ull << -e) - 1)) == 0)) {
        const int neg = d.neg;
        dec_from_u64(d, e >= 0 ? m << e : m >> -e, neg);
        return kPathInteger;
    }
    if (E != 0 && e < 0) {  // a normal non-integer (an integer of 2^(P+1) or more goes to the exact path)
        if (!F32) {
            // (b) Float64, a short decimal d / 10^k with d < 2^50, k <= 22: both are exact
            //     doubles, so the IEEE quotient is the correctly rounded d / 10^k: the string
            //     reads back to x exactly when it equals x. Below 2^50 a float's rounding
            //     interval times 10^k is shorter than 1/4, so level k has at most one such d
            //     and it is the integer nearest the (rounded) product; the first k that has
            //     one therefore gives the only shortest string.
            const u64 a = bits & 0x7fffffffffffffffull;
            double x;
            __builtin_memcpy(&x, &a, 8);
            double t = 1.0;
            for (int k = 1; k <= 22; ++k) {
                t *= 10.0;
                const double p = x * t;
                if (!(p < 1125899906842624.0)) break;  // 2^50
                const u64 di = (u64)(p + 0.5);
                const double dd = (double)di;
                const double diff = p > dd ? p - dd : dd - p;
                if (diff <= p * 4.440892098500626e-16 && di != 0 && dd / t == x) {  // 2^-51
                    const int neg = d.neg;
                    dec_from_u64(d, di, neg);
                    d.pt = d.nd - k;
                    return kPathDecimal;
                }
            }
        } else if (frac != 0) {
            // (b) Float32 in exact double arithmetic: x, the interval's ends (25 bits) and
            //     their products with 10^k = 5^k 2^k (k <= 10: 24 bits) are exact doubles. The
            //     interval is symmetric (frac != 0), so it holds an integer exactly when it
            //     holds the one nearest x 10^k; the first such k gives the shortest string and
            //     that integer is its closest; a tie goes to the even digit.
            const u32 a = (u32)bits & 0x7fffffffu;
            const u32 lo_b = a - 1, hi_b = a + 1;  // (frac != 0, e < 0: both are finite floats)
            float xf, lf, hf;
            __builtin_memcpy(&xf, &a, 4);
            __builtin_memcpy(&lf, &lo_b, 4);
            __builtin_memcpy(&hf, &hi_b, 4);
            const double x = (double)xf;
            const double lo = (x + (double)lf) * 0.5;
            const double hi = (x + (double)hf) * 0.5;
            const bool even = (frac & 1ull) == 0;
            double t = 1.0;
            for (int k = 1; k <= 10; ++k) {
                t *= 10.0;
                const double p = x * t;
                if (!(p < 1099511627776.0)) break;  // 2^40
                const double fl = (double)(u64)p;
                const double rem = p - fl;
                u64 di = (u64)p;
                if (rem > 0.5 || (rem == 0.5 && (di & 1ull))) ++di;
                const double dd = (double)di;
                const double l = lo * t, h = hi * t;
                if (di != 0 && (even ? (dd >= l && dd <= h) : (dd > l && dd < h))) {
                    const int neg = d.neg;
                    dec_from_u64(d, di, neg);
                    d.pt = d.nd - k;
                    return kPathDecimal;
                }
            }
        }
    }
    shortest_exact(d, m, e, frac == 0 && E > 1);
    return kPathExact;
}

// ---------------------------------------------------------------------------
// Positional layout (Rust's Display: never an exponent, no ".0").
DFMI_HD inline int fmt_length(const Dec& d) {
    switch (d.kind) {
        case kInf: return 3 + d.neg;
        case kNaN: return 3;
        case kTrue: return 4;
        case kFalse: return 5;
        default: break;
    }
    if (d.pt >= d.nd) return d.neg + d.pt;      // digits, then zeros
    if (d.pt > 0) return d.neg + d.nd + 1;      // a point inside the digits
    return d.neg + 2 - d.pt + d.nd;             // "0." zeros digits
}
DFMI_HD inline unsigned char fmt_word_byte(u64 packed, int j) { return (unsigned char)(packed >> (8 * j)); }
DFMI_HD inline unsigned char fmt_byte(const Dec& d, int j) {
    if (d.kind == kTrue) return fmt_word_byte(0x65757274ull, j);        // "true"
    if (d.kind == kFalse) return fmt_word_byte(0x65736c6166ull, j);     // "false"
    if (d.kind == kNaN) return fmt_word_byte(0x4e614eull, j);           // "NaN"
    if (d.neg) {
        if (j == 0) return '-';
        --j;
    }
    if (d.kind == kInf) return fmt_word_byte(0x666e69ull, j);           // "inf"
    if (d.pt >= d.nd) return j < d.nd ? (unsigned char)('0' + dec_get(d, j)) : '0';
    if (d.pt > 0) {
        if (j < d.pt) return (unsigned char)('0' + dec_get(d, j));
        return j == d.pt ? '.' : (unsigned char)('0' + dec_get(d, j - 1));
    }
    if (j == 0) return '0';
    if (j == 1) return '.';
    const int i = j - 2 + d.pt;  // (pt <= 0: -pt zeros first)
    return i < 0 ? '0' : (unsigned char)('0' + dec_get(d, i));
}

// A fixed-width value by its dfmi_type and its bits (signed integers sign-extended,
// unsigned zero-extended, Boolean 0 / 1, floats their raw bits). Returns the Path.
DFMI_HD inline int dec_from_value(Dec& d, int type, u64 bits) {
    switch (type) {
        case 1:  // Boolean
            dec_clear(d);
            d.kind = bits ? kTrue : kFalse;
            return kPathSpecial;
        case 2: case 3: case 4: case 5: {  // Int8 .. Int64
            const long long v = (long long)bits;
            dec_from_u64(d, v < 0 ? 0ull - (u64)v : (u64)v, v < 0);
            return kPathInteger;
        }
        case 10: return dec_from_float<true>(d, bits);
        case 11: return dec_from_float<false>(d, bits);
        default:  // UInt8 .. UInt64
            dec_from_u64(d, bits, 0);
            return kPathInteger;
    }
}

// The length alone, for Boolean and the integer types, without their digits.
DFMI_HD inline int fmt_length_int(int type, u64 bits) {
    if (type == 1) return bits ? 4 : 5;
    if (type >= 2 && type <= 5) {
        const long long v = (long long)bits;
        return v < 0 ? 1 + digits10_u64(0ull - (u64)v) : digits10_u64((u64)v);
    }
    return digits10_u64(bits);
}

// Bytes per row that always suffice (include/dfmi.h's table).
DFMI_HD inline int fmt_worst_case(int type) {
    switch (type) {
        case 1: return 5;
        case 2: return 4;
        case 3: return 6;
        case 4: return 11;
        case 5: return 20;
        case 6: return 3;
        case 7: return 5;
        case 8: return 10;
        case 9: return 20;
        case 10: return 48;
        case 11: return 327;
        default: return 0;
    }
}

}  // namespace fmt
}  // namespace dfmi
