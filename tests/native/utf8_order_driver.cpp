// Host-code sanitizer driver (TEST INFRASTRUCTURE) of the Utf8 ordering
// extension (DFMI_FLAG_EXT_UTF8_ORDER). Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_utf8_order_cpu.py, which
// cuts the "utf8 order core" section out of csrc/jit_skeleton.hip into
// utf8_order_core.inc: the text the device compiles is the text run here.
//   1. the comparison core against a bytewise reference: every string in a
//      heap block that ends with the string, at every start alignment mod 8
//      (an over-read is a finding), adversarial pairs and 1e6 random pairs
//      over a small alphabet with long shared prefixes, both head widths;
//   2. the tile pre-pass's aligned head window over a column buffer at every
//      misalignment of its base, the last row ending with the buffer's last
//      aligned word;
//   3. csrc/compile.cpp with the flag on literals that are not NUL-terminated.
// Exit 0 = no finding; the sanitizers abort on the first one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/dfmi.h"

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned char u8;
typedef unsigned u32;

namespace core {
#define DFMI_ORD_FN static inline
#define DFMI_ORD_TAIL static
#define DFMI_ALIGNBYTE(hi, lo, sh) ((u32)(((((u64)(hi)) << 32) | (u64)(lo)) >> (8 * ((sh) & 3u))))
#include "utf8_order_core.inc"
}  // namespace core

namespace {

std::mt19937_64 rng(29);
int rnd(int n) { return (int)(rng() % (uint64_t)n); }

#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
            return 1;                                          \
        }                                                      \
    } while (0)

// The contract, byte by byte: the first differing unsigned byte, else the shorter first.
int reference(const std::string& a, const std::string& b) {
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
        const unsigned char x = (unsigned char)a[i], y = (unsigned char)b[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

// s in a heap block that ends where s ends, starting `align` bytes into it.
struct Exact {
    std::unique_ptr<u8[]> block;
    const u8* p;
    Exact(const std::string& s, int align) : block(new u8[s.size() + (size_t)align]) {
        memcpy(block.get() + align, s.data(), s.size());
        p = block.get() + align;
    }
};

int check_pair(const std::string& a, const std::string& b, int aa, int ab) {
    const Exact x(a, aa), y(b, ab);
    const int want = reference(a, b);
    EXPECT(core::utf8_cmp_bytes<4>(x.p, (int)a.size(), y.p, (int)b.size()) == want);
    EXPECT(core::utf8_cmp_bytes<8>(x.p, (int)a.size(), y.p, (int)b.size()) == want);
    EXPECT(core::utf8_ord<2>(want) == (want < 0) && core::utf8_ord<3>(want) == (want <= 0));
    EXPECT(core::utf8_ord<4>(want) == (want > 0) && core::utf8_ord<5>(want) == (want >= 0));
    return 0;
}

std::vector<std::string> adversarial() {
    std::vector<std::string> d = {"", "a", std::string("a\0", 2), std::string("a\0\0", 3), "ab", "abc", "abcd", "abcde",
                                  "abcdefg", "abcdefgh", "abcdefghi", "abcdefgh\x7f", "abcdefgh\x80", "abcdefgh\xff",
                                  "\xff", "\xe2\x82\xac uro"};
    std::string l40, l200, l300;
    for (int i = 0; i < 300; ++i) l300.push_back((char)('a' + i % 23));
    l40 = l300.substr(0, 40);
    l200 = l300.substr(0, 200);
    for (const std::string& l : {l40, l200, l300}) {
        std::string lo = l, hi = l;
        lo.back() = (char)(l.back() - 1);
        hi.back() = (char)0x80;
        d.insert(d.end(), {l, lo, hi, l.substr(0, l.size() - 1), l + std::string(1, '\0')});
    }
    return d;
}

template <int H>
int check_window(const std::vector<std::string>& rows, const std::vector<std::string>& lits) {
    typedef typename core::Utf8Head<H>::W W;
    std::vector<int> offs(1, 0);
    std::string bytes;
    for (const std::string& r : rows) {
        bytes += r;
        offs.push_back((int)bytes.size());
    }
    for (unsigned bmis = 0; bmis < 4; ++bmis) {
        // the device buffer: 4-aligned words; the block ends with the word of the last byte
        const size_t words = (bmis + bytes.size() + 3) / 4;
        std::unique_ptr<u32[]> block(new u32[words ? words : 1]);
        u8* by = (u8*)block.get() + bmis;
        memcpy(by, bytes.data(), bytes.size());
        for (const std::string& q : lits) {
            const Exact lit(q, 0);
            const int len = (int)q.size(), hq = len < H ? len : H;
            const W qh = core::utf8_head_at<W>(lit.p, hq);
            for (size_t r = 0; r < rows.size(); ++r) {
                const int s = offs[r], L = offs[r + 1] - s;
                const W le = core::utf8_head_window<W>(by - bmis, (unsigned)s + bmis, L < hq ? L : hq);
                int c = core::utf8_cmp_windowed<W>(le, qh, hq, L, len);
                if (c == 2) c = core::utf8_cmp_tail(by + s, L, lit.p, len, H);  // as utf8_cmp_lit_tile goes on
                EXPECT(c == reference(rows[r], q));
            }
        }
    }
    return 0;
}

dfmi_expr_node node(int kind) {
    dfmi_expr_node nd;
    memset(&nd, 0, sizeof nd);
    nd.kind = kind;
    return nd;
}

// The literal lives in a heap block of exactly str_len bytes.
dfmi_expr_node utf8_literal(const std::string& s, std::vector<std::unique_ptr<char[]>>& keep) {
    dfmi_expr_node nd = node(DFMI_EXPR_LITERAL);
    nd.data_type = DFMI_TYPE_UTF8;
    keep.emplace_back(new char[s.size() ? s.size() : 1]);
    memcpy(keep.back().get(), s.data(), s.size());
    nd.str = keep.back().get();
    nd.str_len = (int64_t)s.size();
    return nd;
}

struct Result {
    int32_t rc;
    std::string text;
    int32_t type;
};

Result compile(const std::vector<dfmi_expr_node>& nodes, const dfmi_schema& schema, uint32_t flags) {
    dfmi_program* prog = nullptr;
    dfmi_error err;
    Result r{dfmi_compile_scalar_expr(nodes.data(), (int32_t)nodes.size(), &schema, flags, &prog, &err), "", 0};
    if (r.rc == DFMI_OK) {
        r.text = dfmi_program_name(prog);
        r.type = dfmi_program_type(prog);
        dfmi_program_free(prog);
    } else {
        r.text = err.message;
    }
    return r;
}

int check_compile() {
    dfmi_field fields[3] = {{"s", DFMI_TYPE_UTF8, 1}, {"t", DFMI_TYPE_UTF8, 0}, {"v", DFMI_TYPE_FLOAT64, 1}};
    dfmi_schema schema = {3, 0, fields};
    const uint32_t CMP = DFMI_FLAG_EXT_UTF8_COMPARE, ORD = DFMI_FLAG_EXT_UTF8_ORDER;
    std::vector<std::unique_ptr<char[]>> keep;
    dfmi_expr_node col0 = node(DFMI_EXPR_COLUMN), col1 = node(DFMI_EXPR_COLUMN), col2 = node(DFMI_EXPR_COLUMN);
    col1.column = 1;
    col2.column = 2;
    const char* names[] = {"Lt", "LtEq", "Gt", "GtEq"};
    for (int op = DFMI_OP_LT; op <= DFMI_OP_GT_EQ; ++op) {
        dfmi_expr_node bin = node(DFMI_EXPR_BINARY);
        bin.op = op;
        const std::string nm = names[op - DFMI_OP_LT];
        for (const std::string& lit : {std::string(), std::string("w2"), std::string("a\0b", 3), std::string(200, 'z')}) {
            for (uint32_t fl : {CMP | ORD, CMP}) {  // (without ORDER the node fails only when it runs)
                Result r = compile({col0, utf8_literal(lit, keep), bin}, schema, fl);
                EXPECT(r.rc == DFMI_OK && r.type == DFMI_TYPE_BOOLEAN);
                if (lit.find('\0') == std::string::npos) EXPECT(r.text == "#0 " + nm + " Utf8(\"" + lit + "\")");
                r = compile({utf8_literal(lit, keep), col1, bin}, schema, fl);
                EXPECT(r.rc == DFMI_OK);
                if (lit.find('\0') == std::string::npos) EXPECT(r.text == "Utf8(\"" + lit + "\") " + nm + " #1");
            }
            Result r = compile({col0, utf8_literal(lit, keep), bin}, schema, ORD);  // ORDER alone changes nothing
            EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text.rfind("No support for literal type", 0) == 0);
        }
        Result r = compile({col0, col1, bin}, schema, CMP | ORD);
        EXPECT(r.rc == DFMI_OK && r.type == DFMI_TYPE_BOOLEAN && r.text == "#0 " + nm + " #1");
        r = compile({col0, col2, bin}, schema, CMP | ORD);  // mixed types: compiles, fails when run
        EXPECT(r.rc == DFMI_OK && r.type == DFMI_TYPE_BOOLEAN);
        r = compile({utf8_literal("a", keep), utf8_literal("b", keep), bin}, schema, CMP | ORD);
        EXPECT(r.rc == DFMI_OK && r.type == DFMI_TYPE_BOOLEAN);
        keep.clear();
    }
    return 0;
}

int run() {
    const std::vector<std::string> d = adversarial();
    // 1. adversarial pairs at every pair of start alignments
    for (const std::string& a : d)
        for (const std::string& b : d)
            for (int aa = 0; aa < 8; ++aa)
                for (int ab = 0; ab < 8; ++ab)
                    if (int rc = check_pair(a, b, aa, ab)) return rc;
    // ... and random pairs: alphabet {a, b, 0x00, 0xff}, the second string a
    // prefix or an extension of the first, or equal to it but for one byte
    long n_pairs = 0, n_equal = 0, n_deep = 0;
    const char alpha[4] = {'a', 'b', '\0', '\xff'};
    for (int it = 0; it < 1000000; ++it) {
        std::string a, b;
        const int la = rnd(8) ? rnd(24) : rnd(80);
        for (int i = 0; i < la; ++i) a.push_back(alpha[rnd(rnd(4) ? 2 : 4)]);
        b = a;
        switch (rnd(5)) {
            case 0: b.resize((size_t)rnd(la + 1)); break;
            case 1: for (int i = rnd(6); i > 0; --i) b.push_back(alpha[rnd(4)]); break;
            case 2: if (la) b[(size_t)rnd(la)] = alpha[rnd(4)]; break;
            case 3: if (la) { b.resize((size_t)rnd(la) + 1); b.back() = alpha[rnd(4)]; } break;
            default: break;
        }
        if (int rc = check_pair(a, b, rnd(8), rnd(8))) return rc;
        ++n_pairs;
        n_equal += a == b;
        size_t common = 0;
        while (common < a.size() && common < b.size() && a[common] == b[common]) ++common;
        n_deep += common >= 8 && a != b;
    }
    printf("core: %zu adversarial strings, %ld random pairs (%ld equal, %ld differing past byte 8)\n", d.size(), n_pairs,
           n_equal, n_deep);
    EXPECT(n_equal > 100000 && n_deep > 100000);
    // 2. the tile pre-pass's head window
    std::vector<std::string> rows = d;
    for (int i = 0; i < 200; ++i) rows.push_back(d[(size_t)rnd((int)d.size())]);
    rows.push_back("z");  // the column ends with a one-byte row
    if (int rc = check_window<4>(rows, d)) return rc;
    if (int rc = check_window<8>(rows, d)) return rc;
    rows.pop_back();
    rows.push_back("abcdefgh");  // ... and with a row that fills the last words
    if (int rc = check_window<4>(rows, d)) return rc;
    if (int rc = check_window<8>(rows, d)) return rc;
    // 3. the front end
    return check_compile();
}

}  // namespace

int main() {
    if (int rc = run()) return rc;
    printf("utf8 order driver: clean\n");
    return 0;
}
