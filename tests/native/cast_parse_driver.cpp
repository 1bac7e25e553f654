// Host-code driver (TEST INFRASTRUCTURE) of the string parsers behind CAST
// from Utf8 (DFMI_FLAG_EXT_CAST_ANY). Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_cast_any_cpu.py, which cuts
// the "utf8 parse helpers" section out of csrc/jit_skeleton.hip into
// cast_parse_helpers.inc: the text the device compiles is the text run here.
// Every string is copied into a heap block of exactly its length, so a read
// past either end is a sanitizer finding.
//   - integers and Boolean against a 128-bit restatement of the CSV reader's
//     parse_int and its Boolean rule, for the eight integer types;
//   - Float64 / Float32 against the reader's parse_float (its grammar, then
//     std::from_chars, strtod / strtof beyond the range);
//   - over a fixed corpus and N random strings per kind (argv[1], default
//     300000): random digit strings, %.17g / %.9g of random bit patterns, and
//     random edits of valid strings;
//   - the program limit (st 2) is raised on no string whose digit string,
//     without leading zeros, has at most 19 digits.
// Exit 0 and a closing "clean" line = no finding.
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned char u8;
typedef signed char i8;
typedef short i16;
typedef int i32;
typedef unsigned short u16;
typedef unsigned u32;

namespace core {
#define DFMI_PARSE_FN static inline
#define DFMI_PARSE_OUTLINE static __attribute__((noinline))
#include "cast_parse_helpers.inc"
}  // namespace core

namespace {

std::mt19937_64 rng(47);
long n_int = 0, n_f64 = 0, n_f32 = 0, n_limit = 0, n_null = 0, n_mismatch = 0;

bool lower_eq(const char* b, const char* e, const char* w) {
    const size_t n = strlen(w);
    if ((size_t)(e - b) != n) return false;
    for (size_t i = 0; i < n; ++i)
        if (tolower((unsigned char)b[i]) != w[i]) return false;
    return true;
}

// the reader's parse_int
bool ref_int(const std::string& s, bool is_signed, int bits, u64* v) {
    const char *p = s.data(), *e = p + s.size();
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) {
        neg = *p == '-';
        if (neg && !is_signed) return false;
        ++p;
    }
    if (p == e) return false;
    unsigned __int128 acc = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        acc = acc * 10 + (unsigned)(*p - '0');
        if (acc > ((unsigned __int128)1 << 64)) return false;
    }
    if (is_signed) {
        const unsigned __int128 lim = (unsigned __int128)1 << (bits - 1);
        if (neg ? acc > lim : acc >= lim) return false;
        *v = neg ? 0 - (u64)acc : (u64)acc;
    } else {
        if (bits < 64 ? acc >= ((unsigned __int128)1 << bits) : acc > (unsigned __int128)UINT64_MAX) return false;
        *v = (u64)acc;
    }
    return true;
}

// the reader's parse_float: 0 a parse error, 1 a value (bits); -nan negated (Rust)
template <typename T, typename U>
bool ref_float(const std::string& s, U* bits) {
    const char *p = s.data(), *e = p + s.size();
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
    T x = 0;
    if (lower_eq(p, e, "inf") || lower_eq(p, e, "infinity")) {
        x = INFINITY;
    } else if (lower_eq(p, e, "nan")) {
        *bits = (sizeof(T) == 8 ? (U)0x7FF8000000000000ull : (U)0x7FC00000u) | (neg ? (U)1 << (8 * sizeof(T) - 1) : 0);
        return true;
    } else {
        const char* q = p;
        size_t digits = 0;
        while (q < e && *q >= '0' && *q <= '9') ++q, ++digits;
        if (q < e && *q == '.') {
            ++q;
            while (q < e && *q >= '0' && *q <= '9') ++q, ++digits;
        }
        if (!digits) return false;
        if (q < e && (*q == 'e' || *q == 'E')) {
            ++q;
            if (q < e && (*q == '+' || *q == '-')) ++q;
            size_t ed = 0;
            while (q < e && *q >= '0' && *q <= '9') ++q, ++ed;
            if (!ed) return false;
        }
        if (q != e) return false;
        const auto r = std::from_chars(p, e, x);
        if (r.ec == std::errc::result_out_of_range) {
            const std::string t(p, e);
            x = sizeof(T) == 4 ? (T)strtof(t.c_str(), nullptr) : (T)strtod(t.c_str(), nullptr);
        } else if (r.ec != std::errc() || r.ptr != e) {
            return false;
        }
    }
    if (neg) x = -x;
    memcpy(bits, &x, sizeof(T));
    return true;
}

// digits of the digit string without its leading zeros (0 where it is no plain decimal)
int significant_digits(const std::string& s) {
    int n = 0;
    bool lead = true;
    for (char c : s) {
        if (c == 'e' || c == 'E') break;
        if (c < '0' || c > '9') continue;
        if (lead && c == '0') continue;
        lead = false;
        ++n;
    }
    return n;
}

struct Exact {  // the string in a block of exactly its length
    u8* p;
    int n;
    explicit Exact(const std::string& s) : p((u8*)malloc(s.size() ? s.size() : 1)), n((int)s.size()) {
        if (!s.empty()) memcpy(p, s.data(), s.size());
    }
    ~Exact() { free(p); }
    const u8* data() const { return n ? p : p + 1; }  // an empty string: one past a 1-byte block
};

void show(const std::string& s) {
    fprintf(stderr, "  string (%zu bytes): \"", s.size());
    for (unsigned char c : s) {
        if (c >= 0x20 && c < 0x7f) fputc(c, stderr);
        else fprintf(stderr, "\\x%02x", c);
    }
    fprintf(stderr, "\"\n");
}

int check_ints(const std::string& s) {
    const Exact x(s);
    static const int widths[] = {8, 16, 32, 64};
    for (int sg = 0; sg < 2; ++sg)
        for (int w : widths) {
            u64 want = 0;
            const bool ok = ref_int(s, sg != 0, w, &want);
            const core::ParseRes r = core::parse_int(x.data(), x.n, sg != 0, w);
            ++n_int;
            if (r.st > 1 || (r.st == 1) != ok || (ok && r.bits != want)) {
                fprintf(stderr, "integer mismatch: signed %d width %d: got st %u bits %llx, want ok %d %llx\n", sg, w, r.st,
                        r.bits, (int)ok, want);
                show(s);
                ++n_mismatch;
                return 1;
            }
        }
    const bool t = lower_eq(s.data(), s.data() + s.size(), "true"), f = lower_eq(s.data(), s.data() + s.size(), "false");
    const core::ParseRes b = core::parse_bool(x.data(), x.n);
    if ((b.st == 1) != (t || f) || b.st > 1 || (b.st == 1 && (b.bits != 0) != t)) {
        fprintf(stderr, "Boolean mismatch: got st %u bits %llx\n", b.st, b.bits);
        show(s);
        ++n_mismatch;
        return 1;
    }
    return 0;
}

// expect_limit: -1 do not care (more than 19 digits), 0 / 1 asserted
template <typename T, typename U>
int check_float(const std::string& s, int expect_limit = -1) {
    const Exact x(s);
    U want = 0;
    const bool ok = ref_float<T, U>(s, &want);
    const core::ParseRes r = core::parse_float<T>(x.data(), x.n);
    (sizeof(T) == 8 ? n_f64 : n_f32)++;
    n_null += r.st == 0;
    if (r.st == 2) {
        ++n_limit;
        if (!ok || significant_digits(s) <= 19 || expect_limit == 0) {
            fprintf(stderr, "the program limit on a string that must not reach it (Float%d)\n", 8 * (int)sizeof(T));
            show(s);
            ++n_mismatch;
            return 1;
        }
        return 0;
    }
    if (expect_limit == 1 || r.st > 2 || (r.st == 1) != ok || (ok && (U)r.bits != want) || (r.bits >> (8 * sizeof(T) - 1)) > 1) {
        fprintf(stderr, "Float%d mismatch: got st %u bits %llx, want ok %d %llx%s\n", 8 * (int)sizeof(T), r.st, r.bits,
                (int)ok, (u64)want, expect_limit == 1 ? " (the limit expected)" : "");
        show(s);
        ++n_mismatch;
        return 1;
    }
    return 0;
}

int check_all(const std::string& s) {
    return check_ints(s) | check_float<double, u64>(s) | check_float<float, u32>(s);
}

unsigned rnd(unsigned n) { return (unsigned)(rng() % n); }

std::string random_digits(int max_sig) {
    std::string s;
    if (rnd(4) == 0) s += rnd(2) ? '-' : '+';
    const int lead = rnd(4) == 0 ? (int)rnd(5) : 0;
    const int n = 1 + (int)rnd((unsigned)max_sig);
    std::string d(lead, '0');
    for (int i = 0; i < n; ++i) d += (char)('0' + (i == 0 ? 1 + rnd(9) : rnd(10)));
    if (rnd(3)) {  // a point somewhere (also first or last)
        if (rnd(4) == 0) d = "0." + std::string(rnd(30), '0') + d;  // zeros between the point and the first digit
        else d.insert(rnd((unsigned)d.size() + 1), ".");
    }
    s += d;
    if (rnd(2)) {
        s += rnd(2) ? 'e' : 'E';
        if (rnd(2)) s += rnd(2) ? '-' : '+';
        const unsigned k = rnd(10);
        s += std::to_string(k < 6 ? rnd(40) : k < 9 ? rnd(360) : rnd(100000));
    }
    return s;
}

std::string random_edit(std::string s) {
    static const char alphabet[] = "0123456789+-.eE _xnaifXtruTRUEfalse";
    const int edits = 1 + (int)rnd(2);
    for (int k = 0; k < edits; ++k) {
        const char c = rnd(20) == 0 ? '\0' : alphabet[rnd(sizeof alphabet - 1)];
        const unsigned how = rnd(3);
        if (how == 0 || s.empty()) s.insert(s.begin() + rnd((unsigned)s.size() + 1), c);
        else if (how == 1) s[rnd((unsigned)s.size())] = c;
        else s.erase(s.begin() + rnd((unsigned)s.size()));
    }
    return s;
}

const char* const kCorpus[] = {
    "", "+", "-", "0", "-0", "+0", "007", "-1", "+5", " 5", "5 ", "5.0", "1e3", "1_0", "\xd9\xa3", "true", "TRUE", "False", "t", "1",
    "127", "128", "-128", "-129", "255", "256", "32767", "32768", "-32768", "-32769", "65535", "65536",
    "2147483647", "2147483648", "-2147483648", "-2147483649", "4294967295", "4294967296",
    "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809",
    "18446744073709551615", "18446744073709551616", "18446744073709551617", "1234567890123456789012345678901234567890",
    "1.", ".5", ".", "+.5e-3", "1e", "1e+", "e5", "1e5.0", "0x10", "inf", "-Infinity", "+NaN", "-nan", "infinit", "1e400",
    "-1e-400", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "1.7976931348623158e308",
    "1.7976931348623159e308", "9007199254740993", "16777217.0000000001", "1e0000000000000000005",
    "1e99999999999999999999", "0e99999999999", "9007199254740992.9999999999999999999", "1e-99999999999999999999",
    "3.4028235e38", "3.4028236e38", "1.4e-45", "7e-46", "7.1e-46", "1.17549435e-38", "1e23", "8.5e-309", "1e-309", "123456789012345678e-340",
};

}  // namespace

int main(int argc, char** argv) {
    const long N = argc > 1 ? atol(argv[1]) : 300000;
    int bad = 0;
    for (const char* c : kCorpus) bad |= check_all(c);
    bad |= check_all(std::string("1\0002", 3));
    bad |= check_all(std::string(100, '0') + "1");
    bad |= check_all("0." + std::string(400, '0') + "1");
    bad |= check_all("1" + std::string(30, '0'));
    // the limit itself: the brackets of a 2^53 tie differ for Float64 and agree for Float32
    bad |= check_float<double, u64>("9007199254740993.0000000000000000001", 1);
    bad |= check_float<float, u32>("9007199254740993.0000000000000000001", 0);
    bad |= check_float<double, u64>("9007199254740992.9999999999999999999", 0);
    bad |= check_float<float, u32>("16777217.0000000001", 0);
    if (bad) return 1;

    for (long i = 0; i < N && !bad; ++i) {
        const std::string d = random_digits(19);
        bad |= check_float<double, u64>(d, 0) | check_float<float, u32>(d, 0);
        if (i % 4 == 0) bad |= check_ints(d);
        // digit strings with integer grammar, around every width's range
        {
            std::string s = rnd(3) == 0 ? (rnd(2) ? "-" : "+") : "";
            s += std::string(rnd(4) == 0 ? rnd(4) : 0, '0');
            const int n = 1 + (int)rnd(21);
            for (int k = 0; k < n; ++k) s += (char)('0' + rnd(10));
            bad |= check_ints(s);
        }
        char buf[64];
        u64 b64 = rng();
        double x;
        memcpy(&x, &b64, 8);
        if (std::isfinite(x)) {
            snprintf(buf, sizeof buf, "%.17g", x);
            bad |= check_float<double, u64>(buf, 0) | check_float<float, u32>(buf, 0);
            const std::string e = random_edit(buf);
            bad |= check_float<double, u64>(e) | check_float<float, u32>(e);
            if (i % 4 == 0) bad |= check_ints(e);
        }
        u32 b32 = (u32)rng();
        float f;
        memcpy(&f, &b32, 4);
        if (std::isfinite(f)) {
            snprintf(buf, sizeof buf, "%.9g", (double)f);
            bad |= check_float<float, u32>(buf, 0) | check_float<double, u64>(buf, 0);
        }
        // near the ends of both ranges, where subnormals and overflow live (at most 19 digits)
        snprintf(buf, sizeof buf, "%llue%d", (u64)((rng() >> rnd(64)) % 10000000000000000000ull), (int)rnd(2) ? -(int)(300 + rnd(50)) : (int)(280 + rnd(40)));
        bad |= check_float<double, u64>(buf, 0);
        snprintf(buf, sizeof buf, "%llue%d", (u64)((rng() >> rnd(64)) % 10000000000000000000ull), (int)rnd(2) ? -(int)(25 + rnd(45)) : (int)(15 + rnd(30)));
        bad |= check_float<float, u32>(buf, 0) | check_float<double, u64>(buf, 0);
        // more than 19 digits: the result where the brackets agree, else the limit
        const std::string longd = random_digits(30);
        bad |= check_float<double, u64>(longd) | check_float<float, u32>(longd);
    }
    if (bad || n_mismatch) return 1;
    printf("cast parse driver: %ld integer, %ld Float64, %ld Float32 parses, %ld nulls, %ld at the program limit, "
           "0 mismatches\n", n_int, n_f64, n_f32, n_null, n_limit);
    printf("cast parse driver: clean\n");
    return 0;
}
