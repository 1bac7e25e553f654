// Aggregate extension, host only (agg_host.h): the exact-sum arithmetic, the
// per-row rules of the aggregate kernels restated on the host, the host group
// map with its emission and wire format, and the entry points that never
// touch a device. This is the code that parses bytes received from other
// ranks; tests/native builds it with a plain host compiler under the
// sanitizers.
#include "agg_host.h"

#include "avg_round.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>

namespace dfmi {
namespace aggh {

using namespace layout;

static int agg_fn_of(const std::string& name, uint32_t flags) {
    std::string l = name;
    for (auto& c : l) c = (char)tolower((unsigned char)c);
    if (l == "min") return DFMI_AGG_MIN;
    if (l == "max") return DFMI_AGG_MAX;
    if (l == "count") return DFMI_AGG_COUNT;
    if (l == "sum") return DFMI_AGG_SUM;
    if (l == "avg" && (flags & DFMI_FLAG_EXT_AGG_AVG)) return DFMI_AGG_AVG;
    return -1;
}

bool is_utf8_extreme(const dfmi_aggregate& a) {
    return (a.fn == DFMI_AGG_MIN || a.fn == DFMI_AGG_MAX) && a.arg.type == DFMI_TYPE_UTF8;
}

int acc_fn(const dfmi_aggregate& a) { return is_utf8_extreme(a) ? (int)DFMI_AGG_COUNT : acc_fn(a.fn); }

bool any_utf8_extreme(const dfmi_aggregate* const* aggs, size_t n) {
    for (size_t j = 0; j < n; ++j)
        if (aggs[j] && is_utf8_extreme(*aggs[j])) return true;
    return false;
}

int utf8_compare(const uint8_t* a, size_t la, const uint8_t* b, size_t lb) {
    const size_t n = std::min(la, lb);
    for (size_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return la == lb ? 0 : (la < lb ? -1 : 1);
}

void str_offer(StrVal& v, bool is_min, const uint8_t* s, size_t len) {
    if (v.has) {
        const int c = utf8_compare(s, len, (const uint8_t*)v.s.data(), v.s.size());
        if (is_min ? c >= 0 : c <= 0) return;
    }
    v.has = true;
    v.s.assign((const char*)s, len);
}

bool is_float_type(int t) { return t == DFMI_TYPE_FLOAT32 || t == DFMI_TYPE_FLOAT64; }

bool is_signed_type(int t) {
    return t == DFMI_TYPE_INT8 || t == DFMI_TYPE_INT16 || t == DFMI_TYPE_INT32 || t == DFMI_TYPE_INT64;
}

// GROUP BY keys merged on the host for every batch (no device key window):
// floating-point keys -- one group per bit pattern, ordered by IEEE 754
// totalOrder (Rust's f64::total_cmp: -NaN < -inf < ... < -0.0 < +0.0 < ... <
// +inf < +NaN) -- and Utf8 keys, ordered bytewise (shorter prefix first).
// Build-defined (the reference executes no Aggregate): parity unpinned.
bool host_keyed(int t) { return is_float_type(t) || t == DFMI_TYPE_UTF8; }

// Order value of a non-null Boolean / integer / float key from its bits
// (integers sign/zero-extended, Float32 bits in the low 32).
__int128 key_ord(int t, uint64_t bits) {
    if (t == DFMI_TYPE_FLOAT64) return (__int128)((bits >> 63) ? ~bits : (bits | (1ull << 63)));
    if (t == DFMI_TYPE_FLOAT32) {
        const uint32_t b = (uint32_t)bits;
        return (__int128)((b >> 31) ? (uint32_t)~b : (b | 0x80000000u));
    }
    if (t == DFMI_TYPE_BOOLEAN) return (__int128)bits;
    return is_signed_type(t) ? (__int128)(int64_t)bits : (__int128)bits;
}

// ---- exact merge of accumulator copies (host)
void merge_into(Partial& p, const uint64_t* w, bool is_min) {
    p.count += w[0];
    if ((w[1] & AGGF_VALUE)) {
        if (!(p.flags & AGGF_VALUE)) p.key = w[2];
        else p.key = is_min ? std::min(p.key, w[2]) : std::max(p.key, w[2]);
    }
    p.flags |= w[1];
    p.isum += w[3];
    for (int i = 0; i < kAggLimbs; ++i) p.limbs[i] += (int64_t)w[4 + i];
}

void normalize(Partial& p) {
    for (int i = 0; i < kAggLimbs - 1; ++i) {
        const int64_t c = p.limbs[i] >> 32;  // floor division by 2^32
        p.limbs[i] -= c * 4294967296ll;
        p.limbs[i + 1] += c;
    }
}

// The exact sum (normalised digits, units of 2^-1074) rounded half-to-even
// to a format of `prec` significand bits whose quantum is at least
// 2^(qmin-1074); `zero` when the exact sum is 0. Result as a double (exact
// for Float32 results). With `div` != 0 (AVG): the exact sum divided by `div`
// and rounded once the same way (avg_round.h).
static double round_exact(const Partial& p, int prec, int qmin, double overflow_limit, bool* zero, uint64_t div = 0) {
    // magnitude digits (two's complement negation of the digit string)
    int64_t d[kAggLimbs];
    const bool neg = p.limbs[kAggLimbs - 1] < 0;
    if (!neg) {
        memcpy(d, p.limbs, sizeof d);
    } else {
        int64_t borrow = 0;
        for (int i = 0; i < kAggLimbs; ++i) {
            int64_t v = -p.limbs[i] - borrow;
            borrow = 0;
            if (i < kAggLimbs - 1 && v < 0) {
                v += 4294967296ll;
                borrow = 1;
            }
            d[i] = v;
        }
    }
    int top = -1;
    for (int i = kAggLimbs - 1; i >= 0; --i)
        if (d[i]) {
            top = i;
            break;
        }
    *zero = top < 0;
    if (top < 0) return 0.0;
    if (div) {
        const double v = avg_round_magnitude([&](int i) -> uint32_t { return (uint32_t)d[i]; }, top, div, prec, qmin,
                                             overflow_limit);
        return neg ? -v : v;
    }
    auto bit = [&](int i) -> uint64_t { return i < 0 ? 0 : ((uint64_t)d[i >> 5] >> (i & 31)) & 1; };
    int msb = 32 * top;  // highest set bit (digits < 2^32 after normalisation)
    for (int b = 31; b >= 0; --b)
        if (((uint64_t)d[top] >> b) & 1) {
            msb = 32 * top + b;
            break;
        }
    int q = std::max(msb - (prec - 1), qmin);
    uint64_t mant = 0;  // bits [q, msb] (at most prec <= 53 of them), from the top three digits
    if (q <= msb) {
        const int b0 = std::max(top - 2, 0);
        unsigned __int128 w = 0;
        for (int i = top; i >= b0; --i) w = (w << 32) | (uint64_t)d[i];
        mant = (uint64_t)(w >> (q - 32 * b0)) & ((1ull << (msb - q + 1)) - 1);
    }
    const uint64_t rb = q >= 1 ? bit(q - 1) : 0;
    // sticky: any set bit below the round bit, bits [0, q - 2] (whole digits first)
    bool sticky = false;
    if (q >= 2) {
        const int hb = q - 2, hd = hb >> 5;
        for (int i = 0; i < hd && !sticky; ++i) sticky = d[i] != 0;
        const uint64_t m = (hb & 31) == 31 ? 0xffffffffull : ((1ull << ((hb & 31) + 1)) - 1);
        sticky = sticky || ((uint64_t)d[hd] & m) != 0;
    }
    if (rb && (sticky || (mant & 1))) {
        ++mant;
        if (mant >> prec) {
            mant >>= 1;
            ++q;
        }
    }
    double v = std::ldexp((double)mant, q - 1074);
    if (v >= overflow_limit) v = HUGE_VAL;
    return neg ? -v : v;
}

static uint64_t key_to_bits(uint64_t key, int t) {
    switch (t) {
        case DFMI_TYPE_FLOAT64: return (key >> 63) ? (key & ~(1ull << 63)) : ~key;
        case DFMI_TYPE_FLOAT32: {
            const uint32_t k = (uint32_t)key;
            return (k >> 31) ? (uint64_t)(k & 0x7fffffffu) : (uint64_t)(uint32_t)~k;
        }
        case DFMI_TYPE_INT8: case DFMI_TYPE_INT16: case DFMI_TYPE_INT32: case DFMI_TYPE_INT64:
            return key ^ (1ull << 63);  // the value sign-extended to 64 bits
        default: return key;
    }
}

uint64_t narrow_int(uint64_t v, int t) {
    switch (t) {
        case DFMI_TYPE_INT8: return (uint64_t)(int64_t)(int8_t)v;
        case DFMI_TYPE_INT16: return (uint64_t)(int64_t)(int16_t)v;
        case DFMI_TYPE_INT32: return (uint64_t)(int64_t)(int32_t)v;
        case DFMI_TYPE_UINT8: return v & 0xffull;
        case DFMI_TYPE_UINT16: return v & 0xffffull;
        case DFMI_TYPE_UINT32: return v & 0xffffffffull;
        default: return v;
    }
}

// finish_one of a partial whose digits are already carry-normalised (or, with
// `pre`, of a floating-point SUM whose digits the device has rounded).
dfmi_agg_value finish_normalized(const dfmi_aggregate& a, const Partial& p, const Rounded* pre) {
    dfmi_agg_value r;
    r.type = a.ret_type;
    r.count = (int64_t)p.count;
    r.is_null = 0;
    r.bits = 0;
    const int t = a.arg.type;
    if (a.fn == DFMI_AGG_COUNT) {
        r.bits = p.count;
        return r;
    }
    if (p.count == 0) {
        r.is_null = 1;
        return r;
    }
    if (t == DFMI_TYPE_UTF8) return r;  // a Utf8 MIN / MAX: its caller sets bits, the value's byte length
    const bool f32 = t == DFMI_TYPE_FLOAT32;
    const uint64_t qnan = f32 ? 0x7FC00000ull : 0x7FF8000000000000ull;
    if (a.fn == DFMI_AGG_SUM || a.fn == DFMI_AGG_AVG) {  // (an AVG's argument is a float: dfmi_compile_aggregate)
        const uint64_t div = a.fn == DFMI_AGG_AVG ? p.count : 0;
        if (!is_float_type(t)) {
            r.bits = narrow_int(p.isum, t);
        } else if ((p.flags & AGGF_NAN) || ((p.flags & AGGF_PINF) && (p.flags & AGGF_NINF))) {
            r.bits = qnan;
        } else if (p.flags & (AGGF_PINF | AGGF_NINF)) {
            const bool pos = p.flags & AGGF_PINF;
            r.bits = f32 ? (pos ? 0x7F800000ull : 0xFF800000ull) : (pos ? 0x7FF0000000000000ull : 0xFFF0000000000000ull);
        } else {
            bool zero = false;
            double v;
            if (pre) {
                v = pre->v;
                zero = pre->zero;
            } else {
                v = f32 ? round_exact(p, 24, 925, 0x1p128, &zero, div) : round_exact(p, 53, 0, HUGE_VAL, &zero, div);
            }
            if (zero) v = (p.flags & AGGF_NONNEGZERO) ? 0.0 : -0.0;
            if (f32) {
                const float fv = (float)v;
                uint32_t b;
                memcpy(&b, &fv, 4);
                r.bits = b;
            } else {
                memcpy(&r.bits, &v, 8);
            }
        }
        return r;
    }
    // MIN / MAX
    r.bits = (p.flags & AGGF_VALUE) ? key_to_bits(p.key, t) : qnan;
    return r;
}

dfmi_agg_value finish_one(const dfmi_aggregate& a, Partial p) {
    normalize(p);
    return finish_normalized(a, p);
}

static void merge_partial(Partial& into, const Partial& p, bool is_min) {
    uint64_t w[kAggWords];
    w[0] = p.count;
    w[1] = p.flags;
    w[2] = p.key;
    w[3] = p.isum;
    for (int i = 0; i < kAggLimbs; ++i) w[4 + i] = (uint64_t)p.limbs[i];
    merge_into(into, w, is_min);
}

// The group entry of key `hk` (created with n + 1 empty partials).
GroupState& group_entry(GroupMap& groups, HKey&& hk, size_t n) {
    auto it = groups.find(hk);
    if (it == groups.end()) it = groups.emplace(std::move(hk), GroupState(n + 1)).first;
    return it->second;
}

// One group's state merged into another's: the partials, the hidden row count
// and the Utf8 extremes beside them (one function, so that no merge site can
// take the partials and leave the strings behind).
void merge_group(GroupState& into, const GroupState& parts, const dfmi_aggregate* const* aggs, size_t n) {
    for (size_t j = 0; j < n; ++j) merge_partial(into[j], parts[j], aggs[j]->fn == DFMI_AGG_MIN);
    into[n].count += parts[n].count;  // the hidden count: the group's selected rows
    if (parts.str.empty()) return;
    if (into.str.size() < n) into.str.resize(n);
    for (size_t j = 0; j < n && j < parts.str.size(); ++j)
        if (parts.str[j].has && is_utf8_extreme(*aggs[j]))
            str_offer(into.str[j], aggs[j]->fn == DFMI_AGG_MIN, (const uint8_t*)parts.str[j].s.data(), parts.str[j].s.size());
}

KeyPart fixed_part(int kt, uint64_t bits) {
    KeyPart k;
    k.bits = bits;
    k.ord = key_ord(kt, bits);
    return k;
}

// ---- per-row rules on the host (the host merge: diagnostics A/B, and the
// rows of a batch whose key shares its 63-bit hash with another key's).
// One value (row i, non-null) of aggregate `a` into p -- the per-row rules
// of the aggregate kernels (jit_kernels.cpp generate_agg / generate_agg_grouped,
// jit_skeleton.hip agg_key / agg_sum_flags / fsum_add), restated on the host.
template <typename T>
uint64_t host_agg_key(T v) {
    if constexpr (std::is_same<T, float>::value) {
        uint32_t b;
        memcpy(&b, &v, 4);
        return (b >> 31) ? (uint64_t)(~b) : (uint64_t)(b | 0x80000000u);
    } else if constexpr (std::is_same<T, double>::value) {
        uint64_t b;
        memcpy(&b, &v, 8);
        return (b >> 63) ? ~b : (b | (1ull << 63));
    } else if constexpr (std::is_signed<T>::value) {
        return (uint64_t)(int64_t)v ^ (1ull << 63);
    } else {
        return (uint64_t)v;
    }
}

static void host_fsum_add(Partial& p, double v) {  // finite, non-zero v (fsum_add's digit split)
    uint64_t b;
    memcpy(&b, &v, 8);
    const int e = (int)((b >> 52) & 0x7ff);
    const uint64_t m = (b & ((1ull << 52) - 1)) | (e ? (1ull << 52) : 0ull);
    const int pos = (e ? e : 1) - 1;
    const int d = pos >> 5, sh = pos & 31;
    const uint64_t x0 = (m & 0xffffffffull) << sh, x1 = (m >> 32) << sh;
    int64_t c0 = (int64_t)(x0 & 0xffffffffull);
    int64_t c1 = (int64_t)((x0 >> 32) + (x1 & 0xffffffffull));
    int64_t c2 = (int64_t)(x1 >> 32);
    if (b >> 63) {
        c0 = -c0;
        c1 = -c1;
        c2 = -c2;
    }
    p.limbs[d] += c0;
    p.limbs[d + 1] += c1;
    p.limbs[d + 2] += c2;
}

template <typename T>
void host_accumulate_t(Partial& p, int fn, T v) {
    ++p.count;
    if (fn == DFMI_AGG_COUNT) return;
    if (fn == DFMI_AGG_SUM) {
        if constexpr (std::is_floating_point<T>::value) {
            const unsigned f = v != v ? AGGF_NAN
                                      : (std::isinf(v) ? (v > 0 ? AGGF_PINF : AGGF_NINF)
                                                       : ((v == 0 && std::signbit(v)) ? 0u : AGGF_NONNEGZERO));
            p.flags |= f;
            if (f == AGGF_NONNEGZERO && v != 0) host_fsum_add(p, (double)v);
        } else {
            p.isum += std::is_signed<T>::value ? (uint64_t)(int64_t)v : (uint64_t)v;
        }
        return;
    }
    // MIN / MAX
    if constexpr (std::is_floating_point<T>::value)
        if (v != v) {
            p.flags |= AGGF_NAN;
            return;
        }
    const uint64_t k = host_agg_key(v);
    if (!(p.flags & AGGF_VALUE)) p.key = k;
    else p.key = fn == DFMI_AGG_MIN ? std::min(p.key, k) : std::max(p.key, k);
    p.flags |= AGGF_VALUE;
}

void host_accumulate(Partial& p, int fn, int t, const uint8_t* vals, int64_t i) {
    fn = acc_fn(fn);
    switch (t) {
        case DFMI_TYPE_INT8: return host_accumulate_t(p, fn, ((const int8_t*)vals)[i]);
        case DFMI_TYPE_INT16: return host_accumulate_t(p, fn, ((const int16_t*)vals)[i]);
        case DFMI_TYPE_INT32: return host_accumulate_t(p, fn, ((const int32_t*)vals)[i]);
        case DFMI_TYPE_INT64: return host_accumulate_t(p, fn, ((const int64_t*)vals)[i]);
        case DFMI_TYPE_UINT8: return host_accumulate_t(p, fn, ((const uint8_t*)vals)[i]);
        case DFMI_TYPE_UINT16: return host_accumulate_t(p, fn, ((const uint16_t*)vals)[i]);
        case DFMI_TYPE_UINT32: return host_accumulate_t(p, fn, ((const uint32_t*)vals)[i]);
        case DFMI_TYPE_UINT64: return host_accumulate_t(p, fn, ((const uint64_t*)vals)[i]);
        case DFMI_TYPE_FLOAT32: return host_accumulate_t(p, fn, ((const float*)vals)[i]);
        case DFMI_TYPE_FLOAT64: return host_accumulate_t(p, fn, ((const double*)vals)[i]);
        case DFMI_TYPE_BOOLEAN:  // a bitmap: COUNT, or MIN / MAX over 0 / 1 (DFMI_FLAG_EXT_AGG_MINMAX_ANY)
            return host_accumulate_t(p, fn == DFMI_AGG_SUM ? (int)DFMI_AGG_COUNT : fn, (uint8_t)((vals[i >> 3] >> (i & 7)) & 1));
        default: ++p.count;  // COUNT of a Utf8 argument: non-null values only
    }
}

// Groups in key order as dfmi_agg_state_finish_grouped outputs them:
// keys[g * nkeys + p], values[g * n + j].
void emit_groups(const GroupMap& groups, const std::vector<int>& ktypes, const dfmi_aggregate* const* aggs, size_t n,
                 int64_t cap, dfmi_agg_value* keys, dfmi_agg_value* values, int64_t* num_groups) {
    *num_groups = (int64_t)groups.size();
    if (*num_groups > cap) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "group capacity too small"};
    if (*num_groups > 0 && (!keys || !values)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
    const size_t nk = ktypes.size();
    int64_t g = 0;
    for (const auto& [hk, v] : groups) {
        for (size_t p = 0; p < nk; ++p) {
            dfmi_agg_value& k = keys[g * nk + p];
            const int kt = ktypes[p];
            const KeyPart& kp = hk.p[p];
            k.type = kt;
            k.is_null = kp.null ? 1 : 0;
            k.bits = kp.null || kt == DFMI_TYPE_UTF8 ? 0 : (kt == DFMI_TYPE_BOOLEAN ? kp.bits : narrow_int(kp.bits, kt));
            k.count = (int64_t)v[n].count;  // the group's selected rows
        }
        for (size_t j = 0; j < n; ++j) {
            dfmi_agg_value& out = values[g * n + j];
            out = finish_one(*aggs[j], v[j]);
            if (is_utf8_extreme(*aggs[j]) && !out.is_null) out.bits = j < v.str.size() ? v.str[j].s.size() : 0;
        }
        ++g;
    }
}

// The Utf8 bytes of key part `part` of `groups`, in order, as a BinaryArray.
void emit_key_bytes(const GroupMap& groups, int part, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                    int64_t data_capacity, int64_t* data_length) {
    int64_t total = 0;
    for (const auto& kv : groups) total += (int64_t)kv.first.p[part].s.size();
    *data_length = total;
    if (total > 0x7fffffffll) throw Fail{DFMI_ERR_CAPACITY, "Utf8 group keys of 2^31 bytes or more"};
    if (num_offsets < (int64_t)groups.size() + 1 || data_capacity < total)
        throw Fail{DFMI_ERR_CAPACITY, "key offsets / bytes capacity too small"};
    if (!offsets || (total && !data)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
    int64_t g = 0, pos = 0;
    offsets[0] = 0;
    for (const auto& kv : groups) {
        const std::string& s = kv.first.p[part].s;
        if (!s.empty()) memcpy(data + pos, s.data(), s.size());
        pos += (int64_t)s.size();
        offsets[++g] = (int32_t)pos;
    }
}

void emit_value_bytes(const std::vector<StrVal>& vals, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                      int64_t data_capacity, int64_t* data_length) {
    int64_t total = 0;
    for (const StrVal& v : vals) total += v.has ? (int64_t)v.s.size() : 0;
    *data_length = total;
    if (total > 0x7fffffffll) throw Fail{DFMI_ERR_CAPACITY, "Utf8 aggregate values of 2^31 bytes or more"};
    if (num_offsets < (int64_t)vals.size() + 1 || data_capacity < total)
        throw Fail{DFMI_ERR_CAPACITY, "value offsets / bytes capacity too small"};
    if (!offsets || (total && !data)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
    int64_t g = 0, pos = 0;
    offsets[0] = 0;
    for (const StrVal& v : vals) {
        if (v.has && !v.s.empty()) {
            memcpy(data + pos, v.s.data(), v.s.size());
            pos += (int64_t)v.s.size();
        }
        offsets[++g] = (int32_t)pos;
    }
}

// The values of Utf8 MIN / MAX `agg` of `groups`, in order, as a BinaryArray (a null value's slot empty).
void emit_value_bytes(const GroupMap& groups, int agg, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                      int64_t data_capacity, int64_t* data_length) {
    std::vector<StrVal> vals;
    vals.reserve(groups.size());
    for (const auto& kv : groups)
        vals.push_back((size_t)agg < kv.second.str.size() && kv.second[(size_t)agg].count ? kv.second.str[(size_t)agg] : StrVal{});
    emit_value_bytes(vals, offsets, num_offsets, data, data_capacity, data_length);
}

// Serialised per-group partials (multi-GPU GROUP BY): a header, then per group
// per key part {null, bits, Utf8 length} and the part's bytes (padded to 8),
// then its n + 1 partials (aggregates, then the row count).
struct GroupedHdr {
    uint64_t magic, ngroups, naggs, nkeys;
    int64_t key_types[kMaxKeys];
};
constexpr uint64_t kGroupedMagic = 0x32505247494d4644ull;  // "DFMIGRP2"

size_t grouped_bytes(const GroupMap& groups, size_t n) {
    size_t b = sizeof(GroupedHdr);
    for (const auto& kv : groups) {
        b += (n + 1) * sizeof(Partial);
        for (const KeyPart& k : kv.first.p) b += 24 + (k.s.size() + 7) / 8 * 8;
    }
    return b;
}

void serialize_groups(const GroupMap& groups, const std::vector<int>& ktypes, size_t n, uint8_t* p) {
    GroupedHdr h{};
    h.magic = kGroupedMagic;
    h.ngroups = groups.size();
    h.naggs = n;
    h.nkeys = ktypes.size();
    for (size_t i = 0; i < ktypes.size(); ++i) h.key_types[i] = ktypes[i];
    memcpy(p, &h, sizeof h);
    p += sizeof h;
    for (const auto& [hk, v] : groups) {
        for (const KeyPart& k : hk.p) {
            const uint64_t rec[3] = {k.null ? 1ull : 0ull, k.bits, (uint64_t)k.s.size()};
            memcpy(p, rec, 24);
            p += 24;
            if (!k.s.empty()) memcpy(p, k.s.data(), k.s.size());
            const size_t pad = (k.s.size() + 7) / 8 * 8;
            memset(p + k.s.size(), 0, pad - k.s.size());
            p += pad;
        }
        memcpy(p, v.data(), (n + 1) * sizeof(Partial));
        p += (n + 1) * sizeof(Partial);
    }
}

// Every shard's serialised partials merged into `groups` (key types checked).
void merge_serialized(GroupMap& groups, std::vector<int>& ktypes, const dfmi_aggregate* const* aggs, size_t n,
                      const void* const* partials, const int64_t* sizes, int nparts) {
    for (int r = 0; r < nparts; ++r) {
        const uint8_t* p = (const uint8_t*)partials[r];
        GroupedHdr h;
        if (!p || sizes[r] < (int64_t)sizeof h) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
        memcpy(&h, p, sizeof h);
        if (h.magic != kGroupedMagic || h.naggs != (uint64_t)n || h.nkeys < 1 || h.nkeys > (uint64_t)kMaxKeys)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
        std::vector<int> kt(h.key_types, h.key_types + h.nkeys);
        if (!ktypes.empty() && kt != ktypes) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
        ktypes = kt;
        const uint8_t* end = p + sizes[r];
        p += sizeof h;
        for (uint64_t g = 0; g < h.ngroups; ++g) {
            HKey hk;
            hk.p.resize(h.nkeys);
            for (uint64_t q = 0; q < h.nkeys; ++q) {
                uint64_t rec[3];
                if (end - p < 24) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
                memcpy(rec, p, 24);
                p += 24;
                // (the length is bounded first: rounding a huge one up would wrap)
                if (rec[2] > (uint64_t)(end - p)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
                const size_t pad = (size_t)(rec[2] + 7) / 8 * 8;
                if ((size_t)(end - p) < pad) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
                KeyPart& k = hk.p[q];
                if (rec[0]) {
                    k.null = true;
                } else if (kt[q] == DFMI_TYPE_UTF8) {
                    k.s.assign((const char*)p, (size_t)rec[2]);
                } else {
                    k = fixed_part(kt[q], rec[1]);
                }
                p += pad;
            }
            if ((size_t)(end - p) < (n + 1) * sizeof(Partial)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad grouped partial"};
            GroupState parts(n + 1);
            memcpy(parts.data(), p, (n + 1) * sizeof(Partial));
            p += (n + 1) * sizeof(Partial);
            merge_group(group_entry(groups, std::move(hk), n), parts, aggs, n);
        }
    }
}

}  // namespace aggh
}  // namespace dfmi

using namespace dfmi;
using namespace dfmi::xi;
using namespace dfmi::aggh;

extern "C" int32_t dfmi_compile_aggregate(const char* name, const dfmi_program* arg, int32_t return_type,
                                          uint32_t flags, dfmi_aggregate** out, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!name || !arg || !out) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        // ExecutionContext::execute has no Aggregate arm (context.rs:161)
        if (!(flags & DFMI_FLAG_EXT_AGGREGATE)) throw Fail{DFMI_ERR_PANIC, "not yet implemented"};
        const int fn = agg_fn_of(name, flags);  // compile_expr's match (expression.rs:100-106)
        if (fn < 0) throw Fail{DFMI_ERR_PANIC, std::string("not yet implemented: Unsupported aggregate function '") + name + "'"};
        const int want = fn == DFMI_AGG_COUNT ? DFMI_TYPE_UINT64 : arg->type;  // sqlplanner.rs:296-330
        if (return_type != want) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "aggregate return type does not match the planner's"};
        // DFMI_FLAG_EXT_AGG_MINMAX_ANY: MIN / MAX of a Boolean argument (false < true), kept as an
        // integer extreme over 0 / 1 -- the partial and the wire format are an integer MIN / MAX's
        const bool bool_extreme = (flags & DFMI_FLAG_EXT_AGG_MINMAX_ANY) && arg->type == DFMI_TYPE_BOOLEAN &&
                                  (fn == DFMI_AGG_MIN || fn == DFMI_AGG_MAX);
        // ... and of a Utf8 argument: bytewise order, inside the record machinery a COUNT (agg_host.h acc_fn)
        const bool utf8_extreme = (flags & DFMI_FLAG_EXT_AGG_MINMAX_ANY) && arg->type == DFMI_TYPE_UTF8 &&
                                  (fn == DFMI_AGG_MIN || fn == DFMI_AGG_MAX);
        if (fn != DFMI_AGG_COUNT && !is_numeric_type(arg->type) && !bool_extreme && !utf8_extreme)
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, std::string("aggregate over ") + type_debug(arg->type)};
        // the state keeps only a wrapping 64-bit integer sum: no exact sum to divide
        if (fn == DFMI_AGG_AVG && !is_float_type(arg->type))
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, std::string("AVG over ") + type_debug(arg->type) + ": cast the argument to Float64"};
        dfmi_aggregate* a = new (std::nothrow) dfmi_aggregate();
        if (!a) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "out of memory"};
        a->name = name;
        a->fn = fn;
        a->ret_type = return_type;
        a->arg = *arg;
        *out = a;
        return DFMI_OK;
    });
}

extern "C" const char* dfmi_aggregate_name(const dfmi_aggregate* a) { return a ? a->name.c_str() : ""; }
extern "C" int32_t dfmi_aggregate_type(const dfmi_aggregate* a) { return a ? a->ret_type : 0; }
extern "C" void dfmi_aggregate_free(dfmi_aggregate* a) { delete a; }

extern "C" int32_t dfmi_agg_merge_grouped_partials(const dfmi_aggregate* const* aggs, int32_t n,
                                                   const void* const* partials, const int64_t* sizes, int32_t nparts,
                                                   int64_t cap, dfmi_agg_value* keys, dfmi_agg_value* values,
                                                   int64_t* num_groups, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!aggs || n <= 0 || !partials || !sizes || nparts <= 0 || !num_groups)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        if (any_utf8_extreme(aggs, (size_t)n)) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        GroupMap groups;
        std::vector<int> kt;
        merge_serialized(groups, kt, aggs, (size_t)n, partials, sizes, nparts);
        emit_groups(groups, kt, aggs, (size_t)n, cap, keys, values, num_groups);
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_agg_merge_grouped_partials_keys_utf8(const dfmi_aggregate* const* aggs, int32_t n,
                                                             const void* const* partials, const int64_t* sizes,
                                                             int32_t nparts, int32_t part, int32_t* offsets,
                                                             int64_t num_offsets, uint8_t* data, int64_t data_capacity,
                                                             int64_t* data_length, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!aggs || n <= 0 || !partials || !sizes || nparts <= 0 || !data_length)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        if (any_utf8_extreme(aggs, (size_t)n)) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        GroupMap groups;
        std::vector<int> kt;
        merge_serialized(groups, kt, aggs, (size_t)n, partials, sizes, nparts);
        if (part < 0 || part >= (int32_t)kt.size() || kt[part] != DFMI_TYPE_UTF8)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "not a Utf8 key part"};
        emit_key_bytes(groups, part, offsets, num_offsets, data, data_capacity, data_length);
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_agg_merge_partials(const dfmi_aggregate* const* aggs, int32_t n, const void* const* partials,
                                           int32_t nparts, dfmi_agg_value* out, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!aggs || n <= 0 || !partials || nparts <= 0 || !out) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        if (any_utf8_extreme(aggs, (size_t)n)) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        for (int j = 0; j < n; ++j) {
            Partial m;
            for (int r = 0; r < nparts; ++r) {
                Partial p;
                memcpy(&p, (const uint8_t*)partials[r] + (size_t)j * sizeof(Partial), sizeof p);
                merge_partial(m, p, aggs[j]->fn == DFMI_AGG_MIN);
            }
            out[j] = finish_one(*aggs[j], m);
        }
        return DFMI_OK;
    });
}
