// Query compiler internals shared by jit_expr.cpp (expressions),
// jit_kernels.cpp (kernel bodies) and jit_cache.cpp (compile + caches).
// Not included anywhere else: jit.h is the library's view.
#pragma once
#include <cstdint>
#include <map>
#include <ostream>
#include <string>
#include <tuple>
#include <vector>

#include "dfmi_program.h"
#include "jit.h"

namespace dfmi {
namespace jit {

// FNV-1a, continued from h (kernel names, on-disk cache file names).
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
inline uint64_t fnv1a(const void* p, size_t n, uint64_t h = kFnvBasis) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

const std::string& skeleton_text();  // jit_skeleton.hip, embedded by the Makefile

inline bool is_signed_int(int t) { return t >= DFMI_TYPE_INT8 && t <= DFMI_TYPE_INT64; }

struct Val {
    std::string v;  // C++ expression / local of the node's C++ type (ctype), or bool
    std::string n;  // validity expression ("true" when statically valid)
};

// Expression node -> C++ text, written to *out; literal and string slots.
struct Gen {
    const Plan& P;
    Launch& X;  // slot tables + literal pool being filled
    std::ostream* out;  // where emit writes (emit_predicate points it at the loop's own stream)
    int tmp = 0;
    bool filtered_cols = false;  // projection after a Selection: columns all-valid
    // predicate loop of a filtered tile: Utf8 `col = literal` comparisons are
    // evaluated tile-wide before the loop (utf8_eq_lit_tile); each entry is
    // (array name, utf8 slot, string literal index)
    bool tile_pre = false;
    std::vector<std::tuple<std::string, int, int>> pre_eq;
    // ... and `col <ordering operator> literal` as three-way results
    // (utf8_cmp_lit_tile); the operator is applied in the loop
    std::vector<std::tuple<std::string, int, int>> pre_ord;
    // one literal slot per node however often it is emitted: the aggregate
    // kernel's sub-tile form emits every argument twice (the list pass and the
    // lane-masked pass of a wave whose list overflowed), and a second set of
    // slots would halve the 32 a query may use in that form only
    // (`which`: 0 the node's literal, 1 a literal divisor's reciprocal)
    std::map<std::tuple<const dfmi_program*, int, int>, int> lit_slots;

    Gen(const Plan& p, Launch& x, std::ostream& o) : P(p), X(x), out(&o) {}

    std::string t() { return "t" + std::to_string(tmp++); }
    int lit(uint64_t b);
    int lit_at(const dfmi_program* p, int node, int which, uint64_t b);
    int strlit(const std::string& s);
    // column value for the current row k (inside a per-k loop)
    Val col(const IrNode& n);
    // Emit node i of program p; act = C++ bool expression "row is evaluated".
    Val emit(const dfmi_program* p, int i, int ord_base, const char* act);

private:
    std::string utf8_valid(int u) const;
    Val emit_utf8_order(const dfmi_program* p, const IrNode& n, const IrNode& L, const IrNode& R, int ord_base,
                        const char* act);
    void emit_div_checks(const char* act, const std::string& valid, const Val& a, const Val& b, int ty, int ord,
                         const char* overflow);
};

}  // namespace jit
}  // namespace dfmi
