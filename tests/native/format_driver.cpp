// Host-code driver (TEST INFRASTRUCTURE) of the formatting core behind CAST to
// Utf8 (DFMI_FLAG_EXT_CAST_UTF8). Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_cast_utf8_cpu.py; it
// includes csrc/format_core.h itself: the text the device compiles is the text
// run here. Every value is measured (fmt_length), then written byte by byte
// (fmt_byte) into a heap block of exactly that length, so a disagreement
// between the two passes is a sanitizer finding.
//   - integers against std::to_string: every value of the 8- and 16-bit types,
//     the boundaries and N random values of the wider ones, Boolean;
//   - Float64 / Float32 against std::to_chars(.., chars_format::fixed) (the
//     shortest round-trip form, positional) below 2^53 / 2^24, and from there
//     on -- where that form prints the exact integer, e.g. 1e23 as
//     99999999999999991611392, and Rust's Display 1 and 23 zeros -- against
//     the shortest digits of its scientific form padded with zeros; and,
//     independently, against the
//     smallest p for which strtod / strtof of "%.{p}e" gives the value back
//     (values whose gap below is the gap above; at a power of two the nearest
//     p-digit string may lie outside the shorter half);
//   - over random bit patterns, every power of two, both neighbours of every
//     power of ten, subnormals, both ends of both ranges, integers on both
//     sides of 2^53 / 2^24 and N short decimals (d / 10^k, the fast path).
// argv[1]: N (default 200000). Exit 0 and a closing "clean" line = no finding.
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "format_core.h"

using namespace dfmi::fmt;

namespace {

std::mt19937_64 rng(53);
long n_int = 0, n_f64 = 0, n_f32 = 0, n_mismatch = 0, n_second = 0, longest64 = 0, longest32 = 0;
long paths64[4] = {0, 0, 0, 0}, paths32[4] = {0, 0, 0, 0};

std::string render(const Dec& d) {
    const int n = fmt_length(d);
    char* block = (char*)malloc(n > 0 ? n : 1);  // exactly the measured length
    for (int j = 0; j < n; ++j) block[j] = (char)fmt_byte(d, j);
    std::string s(block, block + n);
    free(block);
    return s;
}

void fail(const char* what, const std::string& got, const std::string& want) {
    if (++n_mismatch <= 20) printf("MISMATCH %s: got '%s' want '%s'\n", what, got.c_str(), want.c_str());
}

void check_int(int type, u64 bits, const std::string& want) {
    Dec d;
    dec_from_value(d, type, bits);
    const std::string got = render(d);
    ++n_int;
    if (got != want) fail("integer", got, want);
    if (fmt_length_int(type, bits) != (int)want.size()) fail("integer length", got, want);
    if ((int)want.size() > fmt_worst_case(type)) fail("integer worst case", got, want);
}

// digits without trailing zeros and the point position of the Dec
void normal_form(const Dec& d, std::string& digits, int& pt) {
    digits.clear();
    for (int i = 0; i < d.nd; ++i) digits.push_back((char)('0' + dec_get(d, i)));
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    pt = d.pt;
}

template <typename F>
void check_float(F v) {
    constexpr bool f32 = sizeof(F) == 4;
    u64 bits = 0;
    memcpy(&bits, &v, sizeof(F));
    Dec d;
    const int path = dec_from_value(d, f32 ? 10 : 11, bits);
    (f32 ? paths32 : paths64)[path]++;
    const std::string got = render(d);
    (f32 ? n_f32 : n_f64)++;
    long& longest = f32 ? longest32 : longest64;
    if ((long)got.size() > longest) longest = (long)got.size();
    if ((int)got.size() > fmt_worst_case(f32 ? 10 : 11)) fail("float worst case", got, "");
    std::string want;
    if (std::isnan(v)) want = "NaN";
    else if (std::isinf(v)) want = v < 0 ? "-inf" : "inf";
    else if (std::fabs((double)v) < (f32 ? 16777216.0 : 9007199254740992.0)) {
        char buf[400];
        auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
        want.assign(buf, r.ptr);
    } else {
        // from 2^53 (2^24) on, to_chars' fixed form prints the float's exact integer value, not
        // its shortest digits; the contract (Rust's Display) pads the shortest digits with
        // zeros. to_chars' shortest digits come from its scientific form: d.ddde+XX
        char buf[64];
        auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
        const std::string s(buf, r.ptr);
        const size_t epos = s.find('e');
        const int ex = atoi(s.c_str() + epos + 1);
        for (size_t i = 0; i < epos; ++i)
            if (s[i] != '.') want.push_back(s[i]);
        const size_t have = want.size() - (want[0] == '-' ? 1 : 0);
        want.append((size_t)ex + 1 - have, '0');
    }
    if (got != want) {
        fail(f32 ? "Float32" : "Float64", got, want);
        return;
    }
    if (std::isnan(v) || std::isinf(v) || v == 0) return;
    // the text reads back to the value
    const std::string z = got;
    if (f32 ? (strtof(z.c_str(), nullptr) != (float)v) : (strtod(z.c_str(), nullptr) != (double)v))
        fail("round trip", got, want);
    // second check: the smallest p whose "%.{p}e" reads back
    const u64 frac = bits & (f32 ? 0x7fffffull : 0xfffffffffffffull);
    if (!frac) return;
    char e[64];
    for (int p = 0; p < 17; ++p) {
        snprintf(e, sizeof e, "%.*e", p, (double)(v < 0 ? -v : v));
        if (f32 ? (strtof(e, nullptr) == (float)(v < 0 ? -v : v)) : (strtod(e, nullptr) == (double)(v < 0 ? -v : v))) break;
    }
    std::string digits;
    const char* q = e;
    for (; *q && *q != 'e'; ++q)
        if (*q != '.') digits.push_back(*q);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int ex = atoi(q + 1);
    std::string mine;
    int pt;
    normal_form(d, mine, pt);
    ++n_second;
    if (mine != digits || pt != ex + 1) fail("second check", mine, digits);
}

template <typename F, typename B>
F from_bits(B b) {
    F v;
    memcpy(&v, &b, sizeof v);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    const long N = argc > 1 ? atol(argv[1]) : 200000;
    // ---- Boolean and integers
    check_int(1, 1, "true");
    check_int(1, 0, "false");
    for (int v = -128; v <= 127; ++v) check_int(2, (u64)(long long)v, std::to_string(v));
    for (int v = 0; v <= 255; ++v) check_int(6, (u64)v, std::to_string(v));
    for (int v = -32768; v <= 32767; ++v) check_int(3, (u64)(long long)v, std::to_string(v));
    for (int v = 0; v <= 65535; ++v) check_int(7, (u64)v, std::to_string(v));
    {
        u64 p = 1;
        for (int k = 0; k < 20; ++k, p *= 10) {  // both sides of every power of ten
            for (u64 v : {p - 1, p, p + 1}) {
                check_int(9, v, std::to_string(v));
                if (v <= (u64)INT64_MAX) {
                    check_int(5, v, std::to_string((long long)v));
                    check_int(5, (u64)(-(long long)v), std::to_string(-(long long)v));
                }
                if (v <= UINT32_MAX) check_int(8, v, std::to_string((uint32_t)v));
                if (v <= (u64)INT32_MAX) {
                    check_int(4, v, std::to_string((int)v));
                    check_int(4, (u64)(long long)(-(int)v), std::to_string(-(int)v));
                }
            }
        }
        check_int(5, (u64)INT64_MIN, std::to_string(INT64_MIN));
        check_int(5, (u64)INT64_MAX, std::to_string(INT64_MAX));
        check_int(9, UINT64_MAX, std::to_string(UINT64_MAX));
        check_int(4, (u64)(long long)INT32_MIN, std::to_string(INT32_MIN));
        check_int(8, UINT32_MAX, std::to_string(UINT32_MAX));
        for (long i = 0; i < N; ++i) {
            const u64 r = rng() >> (rng() % 64);
            check_int(9, r, std::to_string(r));
            check_int(5, r, std::to_string((long long)r));
            check_int(5, 0 - r, std::to_string((long long)(0 - r)));
            check_int(8, (uint32_t)r, std::to_string((uint32_t)r));
            check_int(4, (u64)(long long)(int32_t)r, std::to_string((int32_t)r));
        }
    }
    // ---- floats: the fixed corpus
    for (double v : {0.0, -0.0, 1.0, -1.0, 0.1, 0.5, 1e21, 1e22, 1e23, 5e-324, -5e-324, 2.2250738585072014e-308,
                     2.225073858507201e-308, 1.7976931348623157e308, -1.7976931348623157e308, 9007199254740992.0,
                     9007199254740991.0, 9007199254740993.0, 9007199254740994.0, 0.3, 2.5, 123456.789, 1e-7,
                     4194303.75, 8388607.5, 0.30000000000000004, 1e15, 1e16, 1e17, 123456789012345680.0,
                     (double)INFINITY, -(double)INFINITY, (double)NAN, -(double)NAN}) {
        check_float<double>(v);
        check_float<float>((float)v);
    }
    for (float v : {1e-45f, -1e-45f, 1.17549435e-38f, 1.17549421e-38f, 3.40282347e38f, 16777216.0f, 16777215.0f,
                    16777218.0f, 33554432.0f, 0.1f, 0.3f, 4194303.75f, 8388607.5f, 2097151.875f, 1e10f, 1e-10f})
        check_float<float>(v);
    check_float<double>(from_bits<double, uint64_t>(0x7ff0000000000001ull));  // NaN payloads, both signs
    check_float<double>(from_bits<double, uint64_t>(0xfff8000000000123ull));
    check_float<float>(from_bits<float, uint32_t>(0x7f800001u));
    check_float<float>(from_bits<float, uint32_t>(0xffc00123u));
    for (int e = -1074; e <= 1023; ++e) {  // every power of two and its neighbours
        const double v = ldexp(1.0, e);
        check_float<double>(v);
        check_float<double>(nextafter(v, 0.0));
        check_float<double>(nextafter(v, INFINITY));
    }
    for (int e = -149; e <= 127; ++e) {
        const float v = ldexpf(1.0f, e);
        check_float<float>(v);
        check_float<float>(nextafterf(v, 0.0f));
        check_float<float>(nextafterf(v, INFINITY));
    }
    for (int k = -323; k <= 308; ++k) {  // every power of ten and both neighbours
        char s[32];
        snprintf(s, sizeof s, "1e%d", k);
        const double v = strtod(s, nullptr);
        check_float<double>(v);
        check_float<double>(nextafter(v, 0.0));
        check_float<double>(nextafter(v, INFINITY));
        if (k >= -45 && k <= 38) {
            const float f = strtof(s, nullptr);
            check_float<float>(f);
            check_float<float>(nextafterf(f, 0.0f));
            check_float<float>(nextafterf(f, INFINITY));
        }
    }
    for (uint64_t b = 1; b < 4096; ++b) check_float<double>(from_bits<double, uint64_t>(b));  // subnormals
    for (uint32_t b = 1; b < 4096; ++b) check_float<float>(from_bits<float, uint32_t>(b));
    for (long i = 0; i < 2000; ++i) {  // integers on both sides of the fast path's bound
        check_float<double>(9007199254740992.0 - 1000 + (double)i);
        check_float<double>(9007199254740992.0 + 2.0 * (double)i);
        check_float<float>(16777216.0f - 1000 + (float)i);
        check_float<float>(16777216.0f + 2.0f * (float)i);
    }
    // ---- floats: random
    for (long i = 0; i < N; ++i) {
        check_float<double>(from_bits<double, uint64_t>(rng()));
        check_float<float>(from_bits<float, uint32_t>((uint32_t)rng()));
        check_float<double>(from_bits<double, uint64_t>(rng() & 0x800fffffffffffffull));  // subnormal
        // short decimals: d / 10^k
        const int k = (int)(rng() % 9);
        const u64 dd = rng() >> (20 + rng() % 40);
        double p = 1;
        for (int j = 0; j < k; ++j) p *= 10;
        const double v = (double)dd / p;
        check_float<double>(v);
        check_float<double>(-v);
        check_float<float>((float)((double)(dd % 100000000ull) / p));
        check_float<double>((double)(rng() % 100000) / 100.0);  // two-decimal prices
        check_float<float>((float)(rng() % 100000) / 100.0f);
        check_float<double>((double)(long long)(rng() >> (rng() % 64)));  // integral values
        check_float<float>((float)(long long)(rng() >> (rng() % 64)));
    }
    printf("integers %ld, Float64 %ld (longest %ld), Float32 %ld (longest %ld), second check %ld\n", n_int, n_f64,
           longest64, n_f32, longest32, n_second);
    printf("Float64 paths: special %ld integer %ld decimal %ld exact %ld\n", paths64[0], paths64[1], paths64[2],
           paths64[3]);
    printf("Float32 paths: special %ld integer %ld decimal %ld exact %ld\n", paths32[0], paths32[1], paths32[2],
           paths32[3]);
    printf("mismatches %ld\n", n_mismatch);
    if (n_mismatch) return 1;
    printf("clean\n");
    return 0;
}
