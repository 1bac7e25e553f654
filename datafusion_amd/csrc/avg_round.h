// AVG's finish (DESIGN.md §4 "AVG"): the exact rational (exact sum) / n
// rounded once, half to even -- one text for the host finish (agg_host.cpp
// round_exact) and the device finish (groupby.hip round_digits), in the way
// sort_key.h is shared. Plain C++ with no library call but ldexp, so the host
// sanitizer builds (tests/native) compile it with a host compiler.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DFMI_HD __host__ __device__
#else
#define DFMI_HD
#endif

namespace dfmi {

// |exact sum| / n rounded half to even to `prec` significand bits with a
// quantum of at least 2^(qmin-1074), as a double (exact for a Float32
// result). D(i): digit i of the sum's magnitude in units of 2^-1074, every
// digit in [0, 2^32); `top`: the highest non-zero digit (>= 0: the sum is not
// zero); n in [1, 2^63).
//
// Binary long division from the magnitude's highest set bit downwards, one
// quotient bit per step: the remainder R stays below n < 2^63, so 2R + 1
// fits 64 bits (the device has no 128-by-64 divide). The first quotient 1
// bit fixes the rounding position q; the steps stop at the round bit, q - 1
// -- position -1, a zero dividend bit, when the result's quantum is the
// unit itself: the round bit is then 2R >= n and the tie 2R == n. Whatever
// lies below the round bit is sticky: a non-zero remainder, or any dividend
// bit not yet brought down. So the routine takes about prec + 2 + log2(n)
// steps for every n, and stores no quotient digit.
template <typename Digit>
DFMI_HD inline double avg_round_magnitude(const Digit& D, int top, unsigned long long n, int prec, int qmin,
                                          double overflow_limit) {
    typedef unsigned long long u64_;
    unsigned cur = (unsigned)D(top);
    int hb = 31;
    while (hb > 0 && !((cur >> hb) & 1)) --hb;
    int q = qmin;  // the quantum's bit position; final once the quotient's first 1 bit is known
    bool found = false;
    u64_ R = 0, mant = 0, rb = 0;
    int pos = 32 * top + hb;
    for (; pos >= q - 1; --pos) {
        if (pos >= 0 && (pos & 31) == 31) cur = (unsigned)D(pos >> 5);
        const u64_ bit = pos >= 0 ? (u64_)((cur >> (pos & 31)) & 1u) : 0ull;
        R = (R << 1) | bit;
        const u64_ qb = R >= n ? 1ull : 0ull;
        if (qb) {
            R -= n;
            if (!found) {
                found = true;
                if (pos - (prec - 1) > q) q = pos - (prec - 1);
            }
        }
        if (pos >= q) mant = (mant << 1) | qb;
        else rb = qb;
    }
    // sticky: the remainder, and the dividend bits below the round bit, [0, q - 2] (whole digits first)
    bool sticky = R != 0;
    if (!sticky && q >= 2) {
        const int sb = q - 2, sd = sb >> 5;
        for (int i = 0; i < sd && !sticky; ++i) sticky = (unsigned)D(i) != 0;
        const u64_ m = (sb & 31) == 31 ? 0xffffffffull : ((1ull << ((sb & 31) + 1)) - 1);
        sticky = sticky || ((u64_)(unsigned)D(sd) & m) != 0;
    }
    if (rb && (sticky || (mant & 1))) {
        ++mant;
        if (mant >> prec) {
            mant >>= 1;
            ++q;
        }
    }
    double v = ldexp((double)mant, q - 1074);
    if (v >= overflow_limit) v = (double)INFINITY;
    return v;
}

}  // namespace dfmi
