// Host-code sanitizer driver (TEST INFRASTRUCTURE) for MIN / MAX over a
// Boolean or Utf8 argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY): the aggregate front
// end, the host per-row merge (aggh::host_accumulate over a bitmap; str_offer
// and merge_group for the Utf8 extremes the host group map carries), the
// bytewise comparator against memcmp plus the length rule, the merge and
// finish of Boolean partials (dfmi_agg_merge_partials: an integer MIN / MAX
// partial over 0 / 1) and the refusal of a Utf8 extreme's partial --
// csrc/agg_host.cpp built with AddressSanitizer + UndefinedBehaviorSanitizer
// and compared with brute force.
// Exit 0 = no finding. Built and run by tests/test_minmax_any_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../datafusion_amd/csrc/agg_host.h"
#include "../../include/dfmi.h"

namespace {

using dfmi::aggh::Partial;

std::mt19937_64 rng(77);
uint64_t rnd(uint64_t n) { return rng() % n; }

struct Aggs {
    dfmi_program* prog[2] = {nullptr, nullptr};  // a Boolean column, a Utf8 column
    dfmi_aggregate* mn = nullptr;
    dfmi_aggregate* mx = nullptr;
    dfmi_aggregate* smn = nullptr;  // MIN / MAX of the Utf8 column
    dfmi_aggregate* smx = nullptr;
};

const uint32_t kAgg = DFMI_FLAG_EXT_AGGREGATE;
const uint32_t kAny = DFMI_FLAG_EXT_AGGREGATE | DFMI_FLAG_EXT_AGG_MINMAX_ANY;

// The front end: the flag, the name in any case, the type rule, what stays an error.
int front_end(Aggs& A) {
    dfmi_field fields[2] = {{"b", DFMI_TYPE_BOOLEAN, 1}, {"s", DFMI_TYPE_UTF8, 1}};
    dfmi_schema schema = {2, 0, fields};
    dfmi_error err;
    for (int c = 0; c < 2; ++c) {
        dfmi_expr_node nd;
        memset(&nd, 0, sizeof nd);
        nd.kind = DFMI_EXPR_COLUMN;
        nd.column = c;
        if (dfmi_compile_scalar_expr(&nd, 1, &schema, kAny, &A.prog[c], &err) != DFMI_OK) return 100;
    }
    dfmi_aggregate* bad = nullptr;
    // without both flags: as before
    for (uint32_t fl : {kAgg, kAgg | (uint32_t)DFMI_FLAG_EXT_AGG_AVG}) {
        if (dfmi_compile_aggregate("MIN", A.prog[0], DFMI_TYPE_BOOLEAN, fl, &bad, &err) != DFMI_ERR_NOT_IMPLEMENTED ||
            strcmp(err.message, "aggregate over Boolean"))
            return 101;
    }
    if (dfmi_compile_aggregate("MIN", A.prog[0], DFMI_TYPE_BOOLEAN, DFMI_FLAG_EXT_AGG_MINMAX_ANY, &bad, &err) !=
            DFMI_ERR_PANIC ||
        strcmp(err.message, "not yet implemented"))
        return 102;
    if (dfmi_compile_aggregate("mIn", A.prog[0], DFMI_TYPE_BOOLEAN, kAny, &A.mn, &err) != DFMI_OK) return 103;
    if (dfmi_compile_aggregate("MAX", A.prog[0], DFMI_TYPE_BOOLEAN, kAny, &A.mx, &err) != DFMI_OK) return 104;
    if (strcmp(dfmi_aggregate_name(A.mn), "mIn") || dfmi_aggregate_type(A.mn) != DFMI_TYPE_BOOLEAN ||
        dfmi_aggregate_type(A.mx) != DFMI_TYPE_BOOLEAN)
        return 105;
    for (const char* name : {"SUM", "sum"})
        if (dfmi_compile_aggregate(name, A.prog[0], DFMI_TYPE_BOOLEAN, kAny, &bad, &err) != DFMI_ERR_NOT_IMPLEMENTED ||
            strcmp(err.message, "aggregate over Boolean"))
            return 106;
    if (dfmi_compile_aggregate("avg", A.prog[0], DFMI_TYPE_BOOLEAN, kAny | DFMI_FLAG_EXT_AGG_AVG, &bad, &err) !=
            DFMI_ERR_NOT_IMPLEMENTED ||
        strcmp(err.message, "aggregate over Boolean"))
        return 107;
    for (int32_t rt : {DFMI_TYPE_UINT8, DFMI_TYPE_UINT64, DFMI_TYPE_UTF8})
        if (dfmi_compile_aggregate("MIN", A.prog[0], rt, kAny, &bad, &err) != DFMI_ERR_INVALID_ARGUMENT) return 108;
    // a Utf8 argument: MIN / MAX with both flags; SUM and AVG never
    if (dfmi_compile_aggregate("MAX", A.prog[1], DFMI_TYPE_UTF8, kAgg, &bad, &err) != DFMI_ERR_NOT_IMPLEMENTED ||
        strcmp(err.message, "aggregate over Utf8"))
        return 109;
    for (const char* name : {"SUM", "avg"})
        if (dfmi_compile_aggregate(name, A.prog[1], DFMI_TYPE_UTF8, kAny | DFMI_FLAG_EXT_AGG_AVG, &bad, &err) !=
                DFMI_ERR_NOT_IMPLEMENTED ||
            strcmp(err.message, "aggregate over Utf8"))
            return 110;
    if (dfmi_compile_aggregate("min", A.prog[1], DFMI_TYPE_UTF8, kAny, &A.smn, &err) != DFMI_OK) return 111;
    if (dfmi_compile_aggregate("Max", A.prog[1], DFMI_TYPE_UTF8, kAny, &A.smx, &err) != DFMI_OK) return 112;
    if (dfmi_aggregate_type(A.smn) != DFMI_TYPE_UTF8 || strcmp(dfmi_aggregate_name(A.smx), "Max")) return 113;
    if (dfmi_compile_aggregate("MIN", A.prog[1], DFMI_TYPE_UINT64, kAny, &bad, &err) != DFMI_ERR_INVALID_ARGUMENT) return 114;
    // inside the record machinery a Utf8 extreme is a COUNT
    if (dfmi::aggh::acc_fn(*A.smn) != DFMI_AGG_COUNT || dfmi::aggh::acc_fn(*A.mn) != DFMI_AGG_MIN) return 115;
    printf("front end: pass\n");
    return 0;
}

struct Brute {
    uint64_t count = 0;
    bool any_false = false, any_true = false;
    void add(bool v) {
        ++count;
        (v ? any_true : any_false) = true;
    }
};

int expect(const dfmi_agg_value& v, const Brute& b, bool is_min, int code) {
    if (v.type != DFMI_TYPE_BOOLEAN || v.count != (int64_t)b.count) return code;
    if (!b.count) return v.is_null && v.bits == 0 ? 0 : code + 1;
    const uint64_t want = is_min ? (b.any_false ? 0 : 1) : (b.any_true ? 1 : 0);
    return !v.is_null && v.bits == want ? 0 : code + 2;
}

// Rows of random bitmaps (validity too) merged one by one, as the host merge
// does for the rows of a batch it takes; then the partials of several such
// runs merged and finished through dfmi_agg_merge_partials.
int merges(const Aggs& A) {
    for (int it = 0; it < 3000; ++it) {
        const int nparts = 1 + (int)rnd(4);
        std::vector<Partial> pmin(nparts), pmax(nparts);
        Brute all;
        for (int r = 0; r < nparts; ++r) {
            const int64_t m = (int64_t)rnd(40);  // (an empty run: an empty partial)
            // exactly (m + 7) / 8 bytes each, on the heap: a read past the bitmap is a finding
            std::vector<uint8_t> bits((size_t)(m + 7) / 8), valid((size_t)(m + 7) / 8);
            const int mode = (int)rnd(4);  // random / all false / all true / all null
            for (auto& x : bits) x = mode == 1 ? 0 : (mode == 2 ? 0xff : (uint8_t)rng());
            for (auto& x : valid) x = mode == 3 ? 0 : (uint8_t)(rng() | rng());
            Brute one;
            for (int64_t i = 0; i < m; ++i) {
                if (!((valid[i >> 3] >> (i & 7)) & 1)) continue;
                const bool v = (bits[i >> 3] >> (i & 7)) & 1;
                dfmi::aggh::host_accumulate(pmin[r], DFMI_AGG_MIN, DFMI_TYPE_BOOLEAN, bits.data(), i);
                dfmi::aggh::host_accumulate(pmax[r], DFMI_AGG_MAX, DFMI_TYPE_BOOLEAN, bits.data(), i);
                one.add(v);
                all.add(v);
            }
            // one run finished on its own
            if (int rc = expect(dfmi::aggh::finish_one(*A.mn, pmin[r]), one, true, 200)) return rc;
            if (int rc = expect(dfmi::aggh::finish_one(*A.mx, pmax[r]), one, false, 210)) return rc;
        }
        // both aggregates' partials side by side, as dfmi_agg_state_partial lays them out
        std::vector<std::vector<Partial>> rows(nparts, std::vector<Partial>(2));
        std::vector<const void*> ptr;
        for (int r = 0; r < nparts; ++r) {
            rows[r][0] = pmin[r];
            rows[r][1] = pmax[r];
            ptr.push_back(rows[r].data());
        }
        const dfmi_aggregate* aggs[2] = {A.mn, A.mx};
        dfmi_agg_value out[2];
        dfmi_error err;
        if (dfmi_agg_merge_partials(aggs, 2, ptr.data(), nparts, out, &err) != DFMI_OK) return 220;
        if (int rc = expect(out[0], all, true, 230)) return rc;
        if (int rc = expect(out[1], all, false, 240)) return rc;
    }
    // COUNT of a Boolean argument still only counts
    Partial c;
    const uint8_t byte = 0x5a;
    for (int i = 0; i < 8; ++i) dfmi::aggh::host_accumulate(c, DFMI_AGG_COUNT, DFMI_TYPE_BOOLEAN, &byte, i);
    if (c.count != 8 || c.flags || c.key) return 250;
    printf("merges: 3000 cases, equal to brute force\n");
    return 0;
}

// A random byte string over a small alphabet (0x00, 'a', 0x80, 0xff), exactly `len` heap bytes.
std::vector<uint8_t> random_bytes(size_t len) {
    static const uint8_t alpha[4] = {0x00, 0x61, 0x80, 0xff};
    std::vector<uint8_t> s(len);
    for (auto& c : s) c = alpha[rnd(4)];
    return s;
}

int sign(int x) { return x < 0 ? -1 : (x > 0 ? 1 : 0); }

// memcmp over the common length, then the length rule (a proper prefix is less).
int ref_compare(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    const size_t n = a.size() < b.size() ? a.size() : b.size();
    const int c = n ? memcmp(a.data(), b.data(), n) : 0;
    if (c) return sign(c);
    return a.size() == b.size() ? 0 : (a.size() < b.size() ? -1 : 1);
}

int comparator() {
    using dfmi::aggh::utf8_compare;
    auto cmp = [](const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
        return sign(utf8_compare(a.data(), a.size(), b.data(), b.size()));
    };
    auto lit = [](const char* s, size_t n) { return std::vector<uint8_t>(s, s + n); };
    // hand-built pairs, each a < b
    const std::vector<std::pair<std::vector<uint8_t>, std::vector<uint8_t>>> lt = {
        {lit("", 0), lit("\0", 1)}, {lit("a", 1), lit("a\0", 2)}, {lit("a\x7f", 2), lit("a\x80", 2)},
        {lit("a\xff", 2), lit("b", 1)}, {lit("aaaaaaaa", 8), lit("aaaaaaaa\0", 9)},
        {lit("aaaaaaaa\0", 9), lit("aaaaaaaab", 9)}, {lit("\x7f", 1), lit("\xff", 1)}, {lit("", 0), lit("\xff", 1)}};
    for (const auto& p : lt)
        if (cmp(p.first, p.second) != -1 || cmp(p.second, p.first) != 1 || cmp(p.first, p.first) != 0) return 300;
    for (int it = 0; it < 20000; ++it) {
        std::vector<uint8_t> a = random_bytes(rnd(21)), b = rnd(3) ? random_bytes(rnd(21)) : a;
        if (rnd(4) == 0 && !b.empty()) b.resize(rnd(b.size() + 1));  // a prefix
        if (cmp(a, b) != ref_compare(a, b) || cmp(b, a) != -ref_compare(a, b)) return 301;
    }
    printf("comparator: hand-built pairs and 20000 random pairs equal memcmp + the length rule\n");
    return 0;
}

// The host group map's Utf8 extremes: values offered row by row (str_offer) to
// several groups' states, the states merged (merge_group), against brute
// force; nulls offer nothing, the empty string is a value.
int string_merges(const Aggs& A) {
    using dfmi::aggh::GroupState;
    const dfmi_aggregate* aggs[3] = {A.smn, A.mx, A.smx};  // (a Boolean extreme between them: no string slot used)
    for (int it = 0; it < 2000; ++it) {
        const int nparts = 1 + (int)rnd(4);
        GroupState into(4);
        bool any = false;
        std::vector<uint8_t> lo, hi;
        for (int r = 0; r < nparts; ++r) {
            GroupState part(4);
            if (rnd(5)) part.str.resize(3);  // (a part that saw no string row at all: no slots)
            const int rows = (int)rnd(12);
            for (int i = 0; i < rows && !part.str.empty(); ++i) {
                if (rnd(5) == 0) continue;  // a null
                const std::vector<uint8_t> s = random_bytes(rnd(4) ? rnd(21) : 0);
                dfmi::aggh::str_offer(part.str[0], true, s.data(), s.size());
                dfmi::aggh::str_offer(part.str[2], false, s.data(), s.size());
                if (!any || ref_compare(s, lo) < 0) lo = s;
                if (!any || ref_compare(s, hi) > 0) hi = s;
                any = true;
            }
            dfmi::aggh::merge_group(into, part, aggs, 3);
        }
        const bool has = !into.str.empty() && into.str[0].has;
        if (has != any) return 400;
        if (any) {
            if (!into.str[2].has || into.str[1].has) return 401;
            if (into.str[0].s != std::string(lo.begin(), lo.end()) || into.str[2].s != std::string(hi.begin(), hi.end()))
                return 402;
        }
    }
    // the finish of a Utf8 extreme's partial: type Utf8, count, null when nothing counted (bits: the caller's)
    Partial p;
    dfmi_agg_value v = dfmi::aggh::finish_one(*A.smn, p);
    if (v.type != DFMI_TYPE_UTF8 || !v.is_null || v.count != 0 || v.bits != 0) return 410;
    p.count = 3;
    v = dfmi::aggh::finish_one(*A.smx, p);
    if (v.type != DFMI_TYPE_UTF8 || v.is_null || v.count != 3 || v.bits != 0) return 411;
    printf("string merges: 2000 cases, equal to brute force\n");
    return 0;
}

// The wire format carries no string: every merge of partials given a Utf8 MIN / MAX refuses.
int refusals(const Aggs& A) {
    const char* want = "partial state of a Utf8 MIN / MAX aggregate";
    Partial parts[2];
    const void* ptr[1] = {parts};
    dfmi_agg_value out[2];
    dfmi_error err;
    const dfmi_aggregate* aggs[2] = {A.mn, A.smx};
    if (dfmi_agg_merge_partials(aggs, 2, ptr, 1, out, &err) != DFMI_ERR_NOT_IMPLEMENTED || strcmp(err.message, want)) return 500;
    const int64_t sizes[1] = {(int64_t)sizeof parts};
    int64_t ng = -1;
    int32_t offs[2];
    int64_t len = 0;
    if (dfmi_agg_merge_grouped_partials(aggs, 2, ptr, sizes, 1, 0, nullptr, nullptr, &ng, &err) != DFMI_ERR_NOT_IMPLEMENTED ||
        strcmp(err.message, want))
        return 501;
    if (dfmi_agg_merge_grouped_partials_keys_utf8(aggs, 2, ptr, sizes, 1, 0, offs, 2, nullptr, 0, &len, &err) !=
            DFMI_ERR_NOT_IMPLEMENTED ||
        strcmp(err.message, want))
        return 502;
    printf("refusals: pass\n");
    return 0;
}

}  // namespace

int main() {
    Aggs A;
    int rc = front_end(A);
    if (!rc) rc = merges(A);
    if (!rc) rc = comparator();
    if (!rc) rc = string_merges(A);
    if (!rc) rc = refusals(A);
    dfmi_aggregate_free(A.smn);
    dfmi_aggregate_free(A.smx);
    dfmi_aggregate_free(A.mn);
    dfmi_aggregate_free(A.mx);
    for (dfmi_program* p : A.prog) dfmi_program_free(p);
    if (rc) {
        fprintf(stderr, "minmax any driver: FAILED at %d\n", rc);
        return rc;
    }
    printf("minmax any driver: clean\n");
    return 0;
}
