// Host-code sanitizer driver (TEST INFRASTRUCTURE) for AVG's finish: the
// aggregate front end and the host finish (csrc/agg_host.cpp with
// csrc/avg_round.h, the routine the device finish runs too) built with
// AddressSanitizer + UndefinedBehaviorSanitizer. Partials are built by hand
// (aggh::Partial: count, flags, key, isum, 68 digits in units of 2^-1074,
// not normalised, split over 1 to 3 partials), merged and finished through
// dfmi_agg_merge_partials, and compared bit for bit with an independent
// restatement: a schoolbook division of the whole digit string by n (128-bit
// steps, every quotient digit kept), then one rounding of the quotient with
// the remainder as the sticky bit. Exit 0 = no finding. Built and run by
// tests/test_avg_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../datafusion_amd/csrc/agg_host.h"
#include "../../include/dfmi.h"

namespace {

using dfmi::aggh::Partial;
constexpr int K = dfmi::aggh::layout::kAggLimbs;
constexpr uint64_t F_NAN = 1, F_PINF = 2, F_NINF = 4, F_NNZ = 8;
typedef unsigned __int128 u128;

std::mt19937_64 rng(41);
uint64_t rnd(uint64_t n) { return rng() % n; }

struct Total {  // a signed exact sum: magnitude digits (each < 2^32) and a sign
    uint32_t d[K] = {};
    bool neg = false;
};

// ---- the restatement
// |t| / n rounded half to even to `prec` bits, quantum >= 2^(qmin-1074).
double ref_round(const Total& t, uint64_t n, int prec, int qmin) {
    uint32_t q[K];
    u128 rem = 0;
    for (int i = K - 1; i >= 0; --i) {
        const u128 cur = (rem << 32) | t.d[i];
        q[i] = (uint32_t)(cur / n);
        rem = cur % n;
    }
    auto bit = [&](int i) -> int { return i < 0 ? 0 : (int)((q[i >> 5] >> (i & 31)) & 1u); };
    int msb = -1;
    for (int i = 32 * K - 1; i >= 0 && msb < 0; --i)
        if (bit(i)) msb = i;
    int pos = msb - (prec - 1) > qmin ? msb - (prec - 1) : qmin;  // the quantum
    uint64_t mant = 0;
    for (int i = msb; i >= pos; --i) mant = (mant << 1) | (uint64_t)bit(i);
    int rb;
    bool sticky;
    if (pos == 0) {  // the quantum is the unit: the fraction rem / n against 1/2
        rb = 2 * rem >= n;
        sticky = 2 * rem != n && rem != 0;
    } else {
        rb = bit(pos - 1);
        sticky = rem != 0;
        for (int i = 0; i < pos - 1 && !sticky; ++i) sticky = bit(i);
    }
    if (rb && (sticky || (mant & 1))) {
        ++mant;
        if (mant >> prec) {
            mant >>= 1;
            ++pos;
        }
    }
    return std::ldexp((double)mant, pos - 1074);
}

bool is_zero(const Total& t) {
    for (uint32_t x : t.d)
        if (x) return false;
    return true;
}

// The contract: the result's bits (is_null apart) for total / n with `flags`.
uint64_t ref_bits(const Total& t, uint64_t n, uint64_t flags, bool f32) {
    const uint64_t qnan = f32 ? 0x7FC00000ull : 0x7FF8000000000000ull;
    if ((flags & F_NAN) || ((flags & F_PINF) && (flags & F_NINF))) return qnan;
    if (flags & (F_PINF | F_NINF)) {
        const bool pos = flags & F_PINF;
        return f32 ? (pos ? 0x7F800000ull : 0xFF800000ull) : (pos ? 0x7FF0000000000000ull : 0xFFF0000000000000ull);
    }
    double v;
    if (is_zero(t)) {
        v = (flags & F_NNZ) ? 0.0 : -0.0;
    } else {
        v = f32 ? ref_round(t, n, 24, 925) : ref_round(t, n, 53, 0);
        if (t.neg) v = -v;
    }
    uint64_t b = 0;
    if (f32) {
        const float fv = (float)v;
        uint32_t b4;
        memcpy(&b4, &fv, 4);
        b = b4;
    } else {
        memcpy(&b, &v, 8);
    }
    return b;
}

// ---- partials by hand
// (total, n, flags) over 1 to 3 partials whose digits are not normalised: a
// negative total is the digit-wise negation, and all but the last partial
// hold random digits that the last one takes back.
std::vector<Partial> split(const Total& t, uint64_t n, uint64_t flags) {
    const int parts = 1 + (int)rnd(3);
    std::vector<Partial> p((size_t)parts);
    int64_t left[K];
    for (int i = 0; i < K; ++i) left[i] = t.neg ? -(int64_t)t.d[i] : (int64_t)t.d[i];
    uint64_t nleft = n;
    for (int r = 0; r + 1 < parts; ++r) {
        for (int i = 0; i < K; ++i) {
            const int64_t x = rnd(3) ? (int64_t)rnd(1ull << 40) - (1ll << 39) : 0;
            p[(size_t)r].limbs[i] = x;
            left[i] -= x;
        }
        p[(size_t)r].count = rnd(nleft + 1);
        nleft -= p[(size_t)r].count;
        p[(size_t)r].flags = rnd(2) ? flags : 0;
    }
    for (int i = 0; i < K; ++i) p[(size_t)parts - 1].limbs[i] = left[i];
    p[(size_t)parts - 1].count = nleft;
    p[(size_t)parts - 1].flags = flags;
    return p;
}

struct Aggs {
    dfmi_program* prog[2] = {};
    dfmi_aggregate* agg[2] = {};  // AVG(Float64 column), AVG(Float32 column)
};

int finish(const dfmi_aggregate* a, const std::vector<Partial>& p, dfmi_agg_value* out) {
    std::vector<const void*> ptr;
    for (const Partial& q : p) ptr.push_back(&q);
    dfmi_error err;
    const dfmi_aggregate* aggs[1] = {a};
    return dfmi_agg_merge_partials(aggs, 1, ptr.data(), (int32_t)ptr.size(), out, &err);
}

int check(const Aggs& A, const Total& t, uint64_t n, uint64_t flags, int code) {
    for (int f32 = 0; f32 < 2; ++f32) {
        dfmi_agg_value v;
        if (finish(A.agg[f32], split(t, n, flags), &v) != DFMI_OK) return code;
        if (v.count != (int64_t)n || v.type != (f32 ? DFMI_TYPE_FLOAT32 : DFMI_TYPE_FLOAT64)) return code + 1;
        if (n == 0) {
            if (!v.is_null) return code + 2;
            continue;
        }
        if (v.is_null || v.bits != ref_bits(t, n, flags, f32 != 0)) {
            fprintf(stderr, "case %d f32=%d n=%llu: got %llx want %llx\n", code, f32, (unsigned long long)n,
                    (unsigned long long)v.bits, (unsigned long long)ref_bits(t, n, flags, f32 != 0));
            return code + 3;
        }
    }
    return 0;
}

uint64_t random_n() {
    switch (rnd(5)) {
        case 0: case 1: return 1 + rnd(9);
        case 2: return 1 + rnd(1ull << 32);
        case 3: return (1ull << 32) + rnd((1ull << 62) - (1ull << 32) + 1);
        default: return 1ull << rnd(63);
    }
}

int msb64(uint64_t x) {
    int b = 63;
    while (b > 0 && !((x >> b) & 1)) --b;
    return b;
}

// A mantissa of up to 128 random bits with its highest set bit at `top_bit`.
Total random_total(int top_bit) {
    Total t;
    const int bits = 1 + (int)rnd(128);
    for (int b = 0; b < bits; ++b) {
        const int at = top_bit - b;
        if (at < 0) break;
        if (b == 0 || rnd(2)) t.d[at >> 5] |= 1u << (at & 31);
    }
    t.neg = rnd(5) < 2;
    return t;
}

int random_cases(const Aggs& A) {
    for (int it = 0; it < 6000; ++it) {
        const uint64_t n = random_n();
        // the mean stays finite in Float32 too: |total| / n < 2^(top_bit + 1 - msb(n)) <= 2^(127 + 1074)
        const int hi = 127 + 1074 - 1 + msb64(n);
        int top_bit;
        switch (rnd(4)) {
            case 0: top_bit = (int)rnd(80) + msb64(n); break;          // Float64 subnormal means
            case 1: top_bit = 900 + (int)rnd(80) + msb64(n); break;    // Float32 subnormal means
            default: top_bit = (int)rnd((uint64_t)hi + 1);
        }
        if (top_bit > hi) top_bit = hi;
        if (int rc = check(A, random_total(top_bit), n, F_NNZ, 100)) return rc;
    }
    // Float64 means up to the largest finite value (the Float32 result would be infinite: Float64 only)
    for (int it = 0; it < 2000; ++it) {
        const uint64_t n = random_n();
        const Total t = random_total((int)rnd((uint64_t)(1023 + 1074 - 1 + msb64(n)) + 1));
        dfmi_agg_value v;
        if (finish(A.agg[0], split(t, n, F_NNZ), &v) != DFMI_OK) return 110;
        if (v.is_null || v.count != (int64_t)n || v.bits != ref_bits(t, n, F_NNZ, false)) return 111;
    }
    printf("random: 8000 totals, n up to 2^62, bit-identical to the restatement\n");
    return 0;
}

Total units(uint64_t lo, int shift_bits = 0, bool neg = false) {  // lo << shift_bits
    Total t;
    const u128 w = (u128)lo << (shift_bits & 31);
    const int d0 = shift_bits >> 5;
    for (int i = 0; i < 3; ++i) t.d[d0 + i] = (uint32_t)(w >> (32 * i));
    t.neg = neg;
    return t;
}

int named_cases(const Aggs& A) {
    dfmi_agg_value v;
    // k copies of the largest finite value come back as that value
    for (uint64_t k = 2; k <= 3; ++k) {
        const Total dmax = units(k * ((1ull << 53) - 1), 971 + 1074);
        if (finish(A.agg[0], split(dmax, k, F_NNZ), &v) != DFMI_OK || v.bits != 0x7FEFFFFFFFFFFFFFull) return 200;
        const Total fmax = units(k * ((1ull << 24) - 1), 104 + 1074);
        if (finish(A.agg[1], split(fmax, k, F_NNZ), &v) != DFMI_OK || v.bits != 0x7F7FFFFFull) return 201;
    }
    // 1, 3 and 5 quanta over n = 2: 0 (the tie goes to even), 2, 2 quanta
    const uint64_t want[3] = {0, 2, 2};
    for (int i = 0; i < 3; ++i) {
        if (finish(A.agg[0], split(units(1 + 2 * (uint64_t)i), 2, F_NNZ), &v) != DFMI_OK || v.bits != want[i]) return 210;
        if (finish(A.agg[1], split(units(1 + 2 * (uint64_t)i, 925), 2, F_NNZ), &v) != DFMI_OK || v.bits != want[i])
            return 211;
    }
    // a negative sum whose mean rounds to zero: -0.0
    if (finish(A.agg[0], split(units(1, 0, true), 3, F_NNZ), &v) != DFMI_OK || v.bits != 0x8000000000000000ull) return 220;
    if (finish(A.agg[1], split(units(7, 0, true), 1000, F_NNZ), &v) != DFMI_OK || v.bits != 0x80000000ull) return 221;
    // an exact-zero sum: -0.0 only without AGGF_NONNEGZERO
    if (finish(A.agg[0], split(Total{}, 4, F_NNZ), &v) != DFMI_OK || v.bits != 0) return 230;
    if (finish(A.agg[0], split(Total{}, 4, 0), &v) != DFMI_OK || v.bits != 0x8000000000000000ull) return 231;
    if (finish(A.agg[1], split(Total{}, 4, 0), &v) != DFMI_OK || v.bits != 0x80000000ull) return 232;
    // no value: null; NaN, the infinities, +inf with -inf
    if (int rc = check(A, Total{}, 0, 0, 240)) return rc;
    for (uint64_t fl : {F_NAN | F_NNZ, F_PINF | F_NNZ, F_NINF | F_NNZ, F_PINF | F_NINF | F_NNZ, F_NAN | F_PINF})
        if (int rc = check(A, units(12345, 1000), 7, fl, 250)) return rc;
    // the largest n
    const uint64_t nmax = (1ull << 63) - 1;
    if (int rc = check(A, units(nmax, 1074), nmax, F_NNZ, 260)) return rc;
    if (finish(A.agg[0], split(units(nmax, 1074), nmax, F_NNZ), &v) != DFMI_OK || v.bits != 0x3FF0000000000000ull) return 264;
    if (int rc = check(A, units(1, 1074), nmax, F_NNZ, 270)) return rc;
    printf("named cases: pass\n");
    return 0;
}

// The front end: the flag, the name in any case, the type rule.
int front_end(Aggs& A) {
    dfmi_field fields[3] = {{"x", DFMI_TYPE_FLOAT64, 1}, {"f", DFMI_TYPE_FLOAT32, 1}, {"i", DFMI_TYPE_INT64, 1}};
    dfmi_schema schema = {3, 0, fields};
    const uint32_t fl = DFMI_FLAG_EXT_AGGREGATE | DFMI_FLAG_EXT_AGG_AVG;
    dfmi_error err;
    dfmi_program* pi = nullptr;
    for (int c = 0; c < 3; ++c) {
        dfmi_expr_node nd;
        memset(&nd, 0, sizeof nd);
        nd.kind = DFMI_EXPR_COLUMN;
        nd.column = c;
        if (dfmi_compile_scalar_expr(&nd, 1, &schema, fl, c < 2 ? &A.prog[c] : &pi, &err) != DFMI_OK) return 300;
    }
    const char* names[2] = {"AVG", "aVg"};
    for (int c = 0; c < 2; ++c) {
        if (dfmi_compile_aggregate(names[c], A.prog[c], fields[c].type, fl, &A.agg[c], &err) != DFMI_OK) return 301;
        if (strcmp(dfmi_aggregate_name(A.agg[c]), names[c]) || dfmi_aggregate_type(A.agg[c]) != fields[c].type)
            return 302;
    }
    dfmi_aggregate* bad = nullptr;
    if (dfmi_compile_aggregate("avg", A.prog[0], DFMI_TYPE_FLOAT64, DFMI_FLAG_EXT_AGGREGATE, &bad, &err) != DFMI_ERR_PANIC ||
        strcmp(err.message, "not yet implemented: Unsupported aggregate function 'avg'"))
        return 303;
    if (dfmi_compile_aggregate("avg", pi, DFMI_TYPE_INT64, fl, &bad, &err) != DFMI_ERR_NOT_IMPLEMENTED ||
        strcmp(err.message, "AVG over Int64: cast the argument to Float64"))
        return 304;
    if (dfmi_compile_aggregate("avg", A.prog[0], DFMI_TYPE_FLOAT32, fl, &bad, &err) != DFMI_ERR_INVALID_ARGUMENT) return 305;
    dfmi_program_free(pi);
    return 0;
}

}  // namespace

int main() {
    Aggs A;
    int rc = front_end(A);
    if (!rc) rc = named_cases(A);
    if (!rc) rc = random_cases(A);
    for (int c = 0; c < 2; ++c) {
        dfmi_aggregate_free(A.agg[c]);
        dfmi_program_free(A.prog[c]);
    }
    if (rc) {
        fprintf(stderr, "avg round driver: FAILED at %d\n", rc);
        return rc;
    }
    printf("avg round driver: clean\n");
    return 0;
}
