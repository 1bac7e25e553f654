// Host-code sanitizer driver (TEST INFRASTRUCTURE) of the scalar function
// extension's front end (csrc/compile.cpp, DFMI_FLAG_EXT_SCALAR_FUNCTIONS):
// one function expression compiled, one of each compile error, the registry
// entry point with short / NULL outputs and names that are not
// NUL-terminated, and random function expressions (random names, argument
// counts, types and flags). Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_scalar_fn_sanitize_cpu.py.
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

namespace {

std::mt19937_64 rng(11);
int rnd(int n) { return (int)(rng() % (uint64_t)n); }

const uint32_t FN = DFMI_FLAG_EXT_SCALAR_FUNCTIONS;

dfmi_expr_node column(int c) {
    dfmi_expr_node nd;
    memset(&nd, 0, sizeof nd);
    nd.kind = DFMI_EXPR_COLUMN;
    nd.column = c;
    return nd;
}

// The name lives in a heap block of exactly str_len bytes: a read past it is a finding.
dfmi_expr_node function(const std::string& name, int nargs, int rt, std::vector<std::unique_ptr<char[]>>& keep) {
    dfmi_expr_node nd;
    memset(&nd, 0, sizeof nd);
    nd.kind = DFMI_EXPR_SCALAR_FUNCTION;
    nd.column = nargs;
    nd.data_type = rt;
    keep.emplace_back(new char[name.size() ? name.size() : 1]);
    memcpy(keep.back().get(), name.data(), name.size());
    nd.str = keep.back().get();
    nd.str_len = (int64_t)name.size();
    return nd;
}

struct Result {
    int32_t rc;
    std::string text;  // the program's name, or the error message
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

#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
            return 1;                                             \
        }                                                         \
    } while (0)

int run() {
    dfmi_field fields[4] = {{"i", DFMI_TYPE_INT64, 1}, {"f", DFMI_TYPE_FLOAT64, 1}, {"g", DFMI_TYPE_FLOAT32, 1},
                            {"s", DFMI_TYPE_UTF8, 1}};
    dfmi_schema schema = {4, 0, fields};
    std::vector<std::unique_ptr<char[]>> keep;

    // sqrt(CAST(#0 AS Float64)) and mod(#1, #1)
    dfmi_expr_node cast = column(0);
    cast.kind = DFMI_EXPR_CAST;
    cast.column = 0;
    cast.data_type = DFMI_TYPE_FLOAT64;
    Result r = compile({column(0), cast, function("sqrt", 1, DFMI_TYPE_FLOAT64, keep)}, schema, FN | DFMI_FLAG_EXT_CAST);
    EXPECT(r.rc == DFMI_OK && r.text == "sqrt(CAST(#0 AS Float64))" && r.type == DFMI_TYPE_FLOAT64);
    r = compile({column(1), column(1), function("mod", 2, DFMI_TYPE_FLOAT64, keep)}, schema, FN);
    EXPECT(r.rc == DFMI_OK && r.text == "mod(#1, #1)");
    r = compile({column(2), function("round", 1, DFMI_TYPE_FLOAT32, keep)}, schema, FN);
    EXPECT(r.rc == DFMI_OK && r.type == DFMI_TYPE_FLOAT32);
    // without the flag: the reference's error
    r = compile({column(1), function("sqrt", 1, DFMI_TYPE_FLOAT64, keep)}, schema, 0);
    EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text == "expression sqrt(#1)");
    // one of each error
    r = compile({column(1), function("exp", 1, DFMI_TYPE_FLOAT64, keep)}, schema, FN);
    EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text == "Invalid function 'exp'");
    r = compile({column(1), column(1), function("sqrt", 2, DFMI_TYPE_FLOAT64, keep)}, schema, FN);
    EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text == "Function 'sqrt' expects 1 arguments, got 2");
    r = compile({column(2), column(1), function("mod", 2, DFMI_TYPE_FLOAT64, keep)}, schema, FN);
    EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text == "Function 'mod' is not supported for (Float32, Float64) -> Float64");
    // a NULL name, and a long unknown one (the message is cut to the error frame)
    dfmi_expr_node anon = function("", 1, DFMI_TYPE_FLOAT64, keep);
    anon.str = nullptr;
    anon.str_len = 5;
    r = compile({column(1), anon}, schema, FN);
    EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text == "Invalid function ''");
    r = compile({column(1), function(std::string(2000, 'q'), 1, DFMI_TYPE_FLOAT64, keep)}, schema, FN);
    EXPECT(r.rc == DFMI_ERR_EXECUTION && r.text.size() == sizeof(dfmi_error().message) - 1);

    // the registry entry point
    const char* names[] = {"sqrt", "abs", "floor", "ceil", "round", "trunc", "mod"};
    for (const char* nm : names) {
        int32_t args[2] = {-1, -1}, n = -1, rt = -1;
        const std::string s(nm);
        std::unique_ptr<char[]> exact(new char[s.size()]);
        memcpy(exact.get(), s.data(), s.size());
        EXPECT(dfmi_scalar_function_meta(exact.get(), (int32_t)s.size(), args, 2, &n, &rt) == 0);
        EXPECT(n == (s == "mod" ? 2 : 1) && rt == DFMI_TYPE_FLOAT64 && args[0] == DFMI_TYPE_FLOAT64);
        EXPECT(args[1] == (n == 2 ? DFMI_TYPE_FLOAT64 : -1));
        int32_t one[1] = {-1};
        EXPECT(dfmi_scalar_function_meta(exact.get(), (int32_t)s.size(), one, 1, nullptr, nullptr) == 0);
        EXPECT(dfmi_scalar_function_meta(exact.get(), (int32_t)s.size(), nullptr, 0, nullptr, nullptr) == 0);
        EXPECT(dfmi_scalar_function_meta(exact.get(), (int32_t)s.size() - 1, args, 2, &n, &rt) != 0);  // a prefix
    }
    EXPECT(dfmi_scalar_function_meta(nullptr, 4, nullptr, 0, nullptr, nullptr) != 0);
    EXPECT(dfmi_scalar_function_meta("sqrt", -1, nullptr, 0, nullptr, nullptr) != 0);
    EXPECT(dfmi_scalar_function_meta("SQRT", 4, nullptr, 0, nullptr, nullptr) != 0);

    // random function expressions
    const char* pool[] = {"sqrt", "abs", "floor", "ceil", "round", "trunc", "mod", "exp", "", "sqr", "modx", "MOD"};
    int compiled = 0;
    for (int it = 0; it < 4000; ++it) {
        std::vector<dfmi_expr_node> nodes;
        const int nargs = rnd(4);
        for (int a = 0; a < nargs; ++a) {
            nodes.push_back(column(rnd(3) ? 1 : rnd(5)));  // mostly the Float64 column, sometimes out of range
            if (rnd(3) == 0) {                // a nested function
                nodes.push_back(function(pool[rnd(rnd(3) ? 6 : 12)], 1, DFMI_TYPE_FLOAT32 + (rnd(4) ? 1 : 0), keep));
            }
        }
        dfmi_expr_node f = function(pool[rnd(rnd(3) ? 7 : 12)], rnd(8) ? nargs : rnd(6) - 1, 1 + rnd(12), keep);
        if (rnd(4)) f.data_type = DFMI_TYPE_FLOAT32 + (rnd(4) ? 1 : 0);
        nodes.push_back(f);
        compiled += compile(nodes, schema, (uint32_t)rnd(128) | (rnd(4) ? FN : 0u)).rc == DFMI_OK;
        keep.clear();
    }
    printf("scalar functions: 4000 generated, %d compiled\n", compiled);
    EXPECT(compiled > 50);
    return 0;
}

}  // namespace

int main() {
    if (int rc = run()) return rc;
    printf("scalar function driver: clean\n");
    return 0;
}
