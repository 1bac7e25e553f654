// Host-code sanitizer driver (TEST INFRASTRUCTURE) of the Modulus extension
// (DFMI_FLAG_EXT_MODULUS). Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_modulus_cpu.py, which cuts
// the "modulus helpers" section out of csrc/jit_skeleton.hip into
// modulus_helpers.inc: the text the device compiles is the text run here.
//   1. irem<T> and irem_lit<T> (with csrc/rem_literal.h's reciprocal) against
//      C++ `%`: all pairs of both 8-bit types; every 16-bit x against a list
//      of divisors; for 32 and 64 bits the cross product of an edge set with
//      itself and 1e6 random pairs per width. y = 0 and MIN % -1 (undefined in
//      C++) must give 0 on both paths;
//   2. csrc/compile.cpp over random Modulus expressions with random flags.
// Exit 0 = no finding; the sanitizers abort on the first one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "../../datafusion_amd/csrc/rem_literal.h"
#include "../../include/dfmi.h"

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned char u8;
typedef signed char i8;
typedef short i16;
typedef int i32;
typedef unsigned short u16;
typedef unsigned u32;

namespace core {
#define DFMI_REM_FN static inline
#define DFMI_REM_OUTLINE static __attribute__((noinline))
#include "modulus_helpers.inc"
}  // namespace core

namespace {

std::mt19937_64 rng(31);

#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
            return 1;                                          \
        }                                                      \
    } while (0)

long n_checked = 0, n_undefined = 0, n_corrected = 0;

// One pair on both paths; the literal path's reciprocal as the generator computes it.
template <typename T>
int check(T x, T y) {
    constexpr bool sgn = std::is_signed<T>::value;
    const u64 m = dfmi::rem_reciprocal((int)sizeof(T), sgn, (u64)(i64)y);
    const T g = core::irem<T>(x, y), l = core::irem_lit<T>(x, y, m);
    if (g != l) fprintf(stderr, "%d-byte %s: x=%lld y=%lld general=%lld literal=%lld\n", (int)sizeof(T),
                        sgn ? "signed" : "unsigned", (long long)x, (long long)y, (long long)g, (long long)l);
    EXPECT(g == l);
    if (y == (T)0 || (sgn && y == (T)-1 && x == std::numeric_limits<T>::min())) {
        EXPECT(g == (T)0);
        ++n_undefined;
        return 0;
    }
    T want;
    if constexpr (sizeof(T) < 4) want = (T)((int)x % (int)y);
    else want = (T)(x % y);
    if (g != want) fprintf(stderr, "%d-byte %s: x=%lld y=%lld got=%lld want=%lld\n", (int)sizeof(T),
                           sgn ? "signed" : "unsigned", (long long)x, (long long)y, (long long)g, (long long)want);
    EXPECT(g == want);
    ++n_checked;
    return 0;
}

template <typename T>
int all_pairs_8() {
    for (int x = std::numeric_limits<T>::min(); x <= std::numeric_limits<T>::max(); ++x)
        for (int y = std::numeric_limits<T>::min(); y <= std::numeric_limits<T>::max(); ++y)
            if (int rc = check<T>((T)x, (T)y)) return rc;
    return 0;
}

template <typename T>
int every_x_16() {
    const long long ds[] = {1, -1, 2, -2, 3, -3, 7, -7, 10, -10, 255, -255, 256, -256, 32767, -32767, -32768, 0, 65535};
    for (int x = std::numeric_limits<T>::min(); x <= std::numeric_limits<T>::max(); ++x)
        for (long long d : ds)
            if (int rc = check<T>((T)x, (T)d)) return rc;
    return 0;
}

// A random value of a random magnitude (so that |x| < |y|, |x| ~ |y| and
// |x| >> |y| all occur), either sign for a signed T.
template <typename T>
T random_value() {
    typedef typename std::make_unsigned<T>::type U;
    const int bits = 1 + (int)(rng() % (8 * sizeof(T)));
    U v = (U)rng();
    if (bits < (int)(8 * sizeof(T))) v &= (U)(((U)1 << bits) - 1);
    if (std::is_signed<T>::value && (rng() & 1)) v = (U)0 - v;
    return (T)v;
}

template <typename T>
int wide() {
    const long long MIN = (long long)std::numeric_limits<T>::min();
    const unsigned long long MAX = (unsigned long long)std::numeric_limits<T>::max();
    const unsigned long long p31 = 1ull << 31, p32 = 1ull << 32;
    // (values the type does not hold wrap into it: more edge values, none lost)
    const unsigned long long edge[] = {0, 1, (u64)-1, 2, (u64)-2, (u64)MIN, (u64)MIN + 1, MAX, MAX - 1, p31 - 1, p31,
                                       p31 + 1, (u64)0 - p31 - 1, (u64)0 - p31 + 1, p32 - 1, p32, p32 + 1,
                                       (u64)0 - p32 - 1, (u64)0 - p32 + 1, 3, 7, 10, 255};
    for (unsigned long long x : edge)
        for (unsigned long long y : edge)
            if (int rc = check<T>((T)x, (T)y)) return rc;
    for (int i = 0; i < 1000000; ++i) {
        const T x = random_value<T>(), y = random_value<T>();
        if (int rc = check<T>(x, y)) return rc;
        // ... and x against a small or an extreme divisor, where q^ is most often one short
        const T d = (i & 1) ? (T)(2 + rng() % 1000) : (T)(MAX - rng() % 1000);
        if (int rc = check<T>(x, d)) return rc;
        typedef typename core::RemWord<sizeof(T)>::U U;
        const U ax = (U)x, ad = (U)d;
        if (!std::is_signed<T>::value) {
            const U r = ax - core::rem_mulhi(ax, (U)dfmi::rem_reciprocal((int)sizeof(T), false, (u64)d)) * ad;
            n_corrected += r >= ad;
        }
    }
    return 0;
}

int check_mulhi() {
    for (int i = 0; i < 1000000; ++i) {
        const u64 a = random_value<u64>(), b = random_value<u64>();
        EXPECT(core::rem_mulhi(a, b) == (u64)(((unsigned __int128)a * b) >> 64));
        EXPECT(core::rem_mulhi((u32)a, (u32)b) == (u32)(((u64)(u32)a * (u32)b) >> 32));
    }
    EXPECT(core::rem_mulhi(~0ull, ~0ull) == ~0ull - 1);
    return 0;
}

// ------------------------------------------------------------- the front end
dfmi_expr_node node(int kind) {
    dfmi_expr_node nd;
    memset(&nd, 0, sizeof nd);
    nd.kind = kind;
    return nd;
}

// A random postfix expression of columns, numeric literals and binary
// operators; counts its Modulus nodes. Only "operator: Modulus" can fail it.
void random_expr(int depth, int ncols, std::vector<dfmi_expr_node>& out, int& n_mod) {
    if (depth == 0 || rng() % 4 == 0) {
        if (rng() % 3) {
            dfmi_expr_node c = node(DFMI_EXPR_COLUMN);
            c.column = (int)(rng() % (u64)ncols);
            out.push_back(c);
        } else {
            dfmi_expr_node l = node(DFMI_EXPR_LITERAL);
            if (rng() & 1) {
                l.data_type = DFMI_TYPE_INT64;
                l.i64 = (int64_t)random_value<i64>();
            } else {
                l.data_type = DFMI_TYPE_FLOAT64;
                l.f64 = (double)random_value<i32>() / 8;
            }
            out.push_back(l);
        }
        return;
    }
    random_expr(depth - 1, ncols, out, n_mod);
    random_expr(depth - 1, ncols, out, n_mod);
    dfmi_expr_node b = node(DFMI_EXPR_BINARY);
    static const int ops[] = {DFMI_OP_MODULUS, DFMI_OP_MODULUS, DFMI_OP_PLUS, DFMI_OP_DIVIDE, DFMI_OP_EQ, DFMI_OP_LT,
                              DFMI_OP_AND};
    b.op = ops[rng() % (sizeof ops / sizeof *ops)];
    n_mod += b.op == DFMI_OP_MODULUS;
    out.push_back(b);
}

int check_compile() {
    dfmi_field fields[] = {{"i8", DFMI_TYPE_INT8, 1},   {"i16", DFMI_TYPE_INT16, 0}, {"i32", DFMI_TYPE_INT32, 1},
                           {"i64", DFMI_TYPE_INT64, 1}, {"u8", DFMI_TYPE_UINT8, 0},  {"u16", DFMI_TYPE_UINT16, 1},
                           {"u32", DFMI_TYPE_UINT32, 0}, {"u64", DFMI_TYPE_UINT64, 1}, {"f32", DFMI_TYPE_FLOAT32, 1},
                           {"f64", DFMI_TYPE_FLOAT64, 0}, {"b", DFMI_TYPE_BOOLEAN, 1}, {"s", DFMI_TYPE_UTF8, 1}};
    const int ncols = (int)(sizeof fields / sizeof *fields);
    dfmi_schema schema = {ncols, 0, fields};
    long ok = 0, rejected = 0;
    for (int it = 0; it < 20000; ++it) {
        std::vector<dfmi_expr_node> nodes;
        int n_mod = 0;
        random_expr(1 + (int)(rng() % 4), ncols, nodes, n_mod);
        const uint32_t flags = (uint32_t)(rng() % 0x800);
        dfmi_program* prog = nullptr;
        dfmi_error err;
        const int32_t rc = dfmi_compile_scalar_expr(nodes.data(), (int32_t)nodes.size(), &schema, flags, &prog, &err);
        if (n_mod && !(flags & DFMI_FLAG_EXT_MODULUS)) {
            EXPECT(rc == DFMI_ERR_EXECUTION && prog == nullptr && !strcmp(err.message, "operator: Modulus"));
            ++rejected;
        } else {
            EXPECT(rc == DFMI_OK && prog != nullptr);
            const std::string name = dfmi_program_name(prog);
            EXPECT((name.find(" Modulus ") != std::string::npos) == (n_mod > 0));
            dfmi_program_free(prog);
            ++ok;
        }
    }
    printf("front end: %ld compiled, %ld rejected without the flag\n", ok, rejected);
    EXPECT(ok > 5000 && rejected > 2000);
    return 0;
}

int run() {
    if (int rc = check_mulhi()) return rc;
    if (int rc = all_pairs_8<i8>()) return rc;
    if (int rc = all_pairs_8<u8>()) return rc;
    if (int rc = every_x_16<i16>()) return rc;
    if (int rc = every_x_16<u16>()) return rc;
    if (int rc = wide<i32>()) return rc;
    if (int rc = wide<u32>()) return rc;
    if (int rc = wide<i64>()) return rc;
    if (int rc = wide<u64>()) return rc;
    printf("remainder: %ld pairs against %%, %ld undefined pairs (0 on both paths), %ld one-step corrections seen\n",
           n_checked, n_undefined, n_corrected);
    EXPECT(n_checked > 8000000 && n_undefined > 500 && n_corrected > 1000);
    return check_compile();
}

}  // namespace

int main() {
    if (int rc = run()) return rc;
    printf("modulus driver: clean\n");
    return 0;
}
