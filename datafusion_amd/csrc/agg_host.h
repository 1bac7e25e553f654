// Aggregate extension, the part with no device in it (agg_host.cpp): the
// exact-sum arithmetic and per-row rules restated on the host, the host's
// group map, and the wire format of the partials that ranks exchange. Builds
// with a plain host compiler (tests/native runs it under the sanitizers).
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "dfmi_program.h"

namespace dfmi {
namespace aggh {

// The accumulator layout, restated: the device code defines it
// (jit_skeleton.hip, groupby.h; the skeleton is also hipRTC text and cannot
// include this file). agg_hash.cpp, which sees both, asserts they are equal.
namespace layout {
constexpr int kAggCopies = 64;
constexpr int kAggLimbs = 68;
constexpr int kAggWords = 4 + kAggLimbs;
enum AggFlag : unsigned { AGGF_NAN = 1, AGGF_PINF = 2, AGGF_NINF = 4, AGGF_NONNEGZERO = 8, AGGF_VALUE = 16 };
constexpr unsigned long long kRoundZero = 1ull << 32;
constexpr int kMaxKeys = 4;
}  // namespace layout

// One aggregate's merged state (host): the layout of a device copy with the
// float digits carry-normalised (every digit but the top in [0, 2^32)).
struct Partial {
    uint64_t count = 0, flags = 0, key = 0, isum = 0;
    int64_t limbs[layout::kAggLimbs] = {};
};

// GROUP BY keys on the host: one part per key expression, ordered
// lexicographically, each part with its null last (emit_groups' order; the
// oracle's group_key). A non-null part orders by `ord` (key_ord: integers
// numerically, Boolean false < true, floats by IEEE 754 totalOrder), then by
// its bytes (Utf8: bytewise, a shorter prefix first).
struct KeyPart {
    bool null = false;
    __int128 ord = 0;
    uint64_t bits = 0;  // Boolean 0/1, integers sign/zero-extended, float bits
    std::string s;      // Utf8
};
struct HKey {
    std::vector<KeyPart> p;
    bool operator<(const HKey& o) const {
        for (size_t i = 0; i < p.size(); ++i) {
            const KeyPart &a = p[i], &b = o.p[i];
            if (a.null != b.null) return !a.null;
            if (a.null) continue;
            if (a.ord != b.ord) return a.ord < b.ord;
            if (a.s != b.s) return a.s < b.s;
        }
        return false;
    }
};
// A Utf8 MIN / MAX's extreme string on the host (none yet: !has). The bytes
// travel beside the Partial, which the wire format copies with memcpy and
// which therefore stays trivially copyable.
struct StrVal {
    bool has = false;
    std::string s;
};
// A group's partials (+ its row count) and, beside them, the extreme of each
// Utf8 MIN / MAX (str[j], sized on first use; empty without one).
struct GroupState : std::vector<Partial> {
    using std::vector<Partial>::vector;
    explicit GroupState(std::vector<Partial>&& v) : std::vector<Partial>(std::move(v)) {}
    std::vector<StrVal> str;
};
using GroupMap = std::map<HKey, GroupState>;  // key -> partials + the group's row count

// A floating-point SUM already rounded (the device finish, k_group_round).
struct Rounded {
    double v;
    bool zero;
};

// The function an aggregate ACCUMULATES as: an AVG's state is a float SUM's
// (exact digits and the non-null count); only the finish divides. Kernels,
// generated sources and their cache keys see SUM, so SUM(e) and AVG(e) share
// one code object.
inline int acc_fn(int fn) { return fn == DFMI_AGG_AVG ? DFMI_AGG_SUM : fn; }
// ... and a MIN / MAX over a Utf8 argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY)
// accumulates as COUNT: the record machinery tracks its count / null and
// shares COUNT's code objects; the strings live beside it (str_extreme.h on
// the device, GroupState::str on the host) and the finish joins the two.
// (the wire format ranks exchange carries no string: every partial entry point refuses one)
constexpr const char* kUtf8ExtremePartial = "partial state of a Utf8 MIN / MAX aggregate";
bool is_utf8_extreme(const dfmi_aggregate& a);
int acc_fn(const dfmi_aggregate& a);
bool any_utf8_extreme(const dfmi_aggregate* const* aggs, size_t n);
// < 0, 0, > 0: two byte strings as sequences of unsigned bytes, the first
// differing byte decides, a proper prefix is less (the GROUP BY / ORDER BY order).
int utf8_compare(const uint8_t* a, size_t la, const uint8_t* b, size_t lb);
// One value offered to an extreme (is_min: keeps the lesser).
void str_offer(StrVal& v, bool is_min, const uint8_t* s, size_t len);

bool is_float_type(int t);
bool is_signed_type(int t);
bool host_keyed(int t);
__int128 key_ord(int t, uint64_t bits);
uint64_t narrow_int(uint64_t v, int t);
void merge_into(Partial& p, const uint64_t* w, bool is_min);
void normalize(Partial& p);
dfmi_agg_value finish_normalized(const dfmi_aggregate& a, const Partial& p, const Rounded* pre = nullptr);
dfmi_agg_value finish_one(const dfmi_aggregate& a, Partial p);
void host_accumulate(Partial& p, int fn, int t, const uint8_t* vals, int64_t i);

KeyPart fixed_part(int kt, uint64_t bits);
GroupState& group_entry(GroupMap& groups, HKey&& hk, size_t n);
void emit_value_bytes(const GroupMap& groups, int agg, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                      int64_t data_capacity, int64_t* data_length);
// The same from values in output order (null: !has).
void emit_value_bytes(const std::vector<StrVal>& vals, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                      int64_t data_capacity, int64_t* data_length);
void merge_group(GroupState& into, const GroupState& parts, const dfmi_aggregate* const* aggs, size_t n);
void emit_groups(const GroupMap& groups, const std::vector<int>& ktypes, const dfmi_aggregate* const* aggs, size_t n,
                 int64_t cap, dfmi_agg_value* keys, dfmi_agg_value* values, int64_t* num_groups);
void emit_key_bytes(const GroupMap& groups, int part, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                    int64_t data_capacity, int64_t* data_length);
size_t grouped_bytes(const GroupMap& groups, size_t n);
void serialize_groups(const GroupMap& groups, const std::vector<int>& ktypes, size_t n, uint8_t* p);
void merge_serialized(GroupMap& groups, std::vector<int>& ktypes, const dfmi_aggregate* const* aggs, size_t n,
                      const void* const* partials, const int64_t* sizes, int nparts);

}  // namespace aggh
}  // namespace dfmi

struct dfmi_aggregate {
    std::string name;  // as spelled in the SQL text (the Field name, sqlplanner.rs:385-389)
    int fn = 0;        // dfmi_agg_fn
    int ret_type = 0;
    dfmi_program arg;  // compile_expr's compiled argument (a copy: same uid, same kernels)
};
