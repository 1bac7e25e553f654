// Host-code sanitizer driver (TEST INFRASTRUCTURE): the library's host-only
// front ends -- the expression compiler (csrc/compile.cpp) and the CSV
// reader (csrc/csv_reader.cpp) and the aggregate extension's host-only part
// (csrc/agg_host.cpp: exact-sum arithmetic, the host group map, the partials
// that ranks exchange) and the host paths' device-free parts (bitmap
// splicing, the worker pool, the chunk and host-batches layouts:
// csrc/host_bits.h, host_pool.h, host_plan.cpp) -- plus the CPU oracle, built with
// AddressSanitizer + UndefinedBehaviorSanitizer and driven over random
// expressions, random batches, generated CSV files (quotes, CRLF, empty
// and missing fields, bad numbers), random aggregates merged from serialised
// partials and compared bit for bit with the oracle, and malformed partials.
// Exit 0 = no finding; the sanitizers abort on the first one. Built and run
// by tests/test_sanitize_cpu.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../datafusion_amd/csrc/agg_host.h"
#include "../../datafusion_amd/csrc/col_layout.h"
#include "../../datafusion_amd/csrc/host_bits.h"
#include "../../datafusion_amd/csrc/host_plan.h"
#include "../../datafusion_amd/csrc/host_pool.h"
#include "../../include/dfmi.h"
#include "../../include/dfmi_datasource.h"
#include "../../oracle/oracle.h"

namespace {

std::mt19937_64 rng(7);
int rnd(int n) { return (int)(rng() % (uint64_t)n); }

const int kTypes[] = {DFMI_TYPE_INT64, DFMI_TYPE_FLOAT64, DFMI_TYPE_INT32, DFMI_TYPE_FLOAT32, DFMI_TYPE_UTF8,
                      DFMI_TYPE_BOOLEAN, DFMI_TYPE_UINT8};
constexpr int kCols = 7;

// A random postfix expression over the schema (any shape: the compilers
// must reject what the reference rejects without misbehaving).
void gen(std::vector<dfmi_expr_node>& out, int depth, std::vector<std::string>& strs) {
    dfmi_expr_node nd;
    memset(&nd, 0, sizeof nd);
    const int r = rnd(10);
    if (depth == 0 || r < 3) {
        if (rnd(2)) {
            nd.kind = DFMI_EXPR_COLUMN;
            nd.column = rnd(kCols + 1) - (rnd(20) == 0 ? 3 : 0);  // sometimes out of range
        } else {
            nd.kind = DFMI_EXPR_LITERAL;
            nd.data_type = 1 + rnd(12);
            nd.i64 = (int64_t)rng();
            nd.f64 = (double)(int64_t)rng() / 1e9;
            if (nd.data_type == DFMI_TYPE_UTF8) {
                strs.push_back(std::string(rnd(6), 'a' + rnd(3)));
                nd.str = strs.back().c_str();
                nd.str_len = (int64_t)strs.back().size();
            }
        }
        out.push_back(nd);
        return;
    }
    if (r < 8) {
        gen(out, depth - 1, strs);
        gen(out, depth - 1, strs);
        nd.kind = DFMI_EXPR_BINARY;
        nd.op = rnd(13);
    } else if (r < 9) {
        gen(out, depth - 1, strs);
        nd.kind = DFMI_EXPR_CAST;
        nd.data_type = 1 + rnd(12);
    } else {
        gen(out, depth - 1, strs);
        nd.kind = rnd(2) ? DFMI_EXPR_IS_NULL : DFMI_EXPR_IS_NOT_NULL;
    }
    out.push_back(nd);
}

int check_expressions() {
    dfmi_field fields[kCols];
    const char* names[kCols] = {"i", "f", "i32", "f32", "s", "b", "u8"};
    for (int c = 0; c < kCols; ++c) fields[c] = {names[c], kTypes[c], 1};
    dfmi_schema schema = {kCols, 0, fields};
    // a random 300-row batch with nulls
    const int n = 300;
    std::vector<int64_t> vi(n);
    std::vector<double> vf(n);
    std::vector<int32_t> vi32(n), offs(n + 1);
    std::vector<float> vf32(n);
    std::vector<uint8_t> vu8(n), bits((n + 63) / 64 * 8), valid((n + 63) / 64 * 8);
    std::string bytes;
    for (int r = 0; r < n; ++r) {
        vi[r] = (int64_t)rng() >> rnd(60);
        vf[r] = (double)(int64_t)rng() / 1e12;
        vi32[r] = (int32_t)rng();
        vf32[r] = (float)vf[r];
        vu8[r] = (uint8_t)rng();
        offs[r] = (int32_t)bytes.size();
        bytes += std::string(rnd(5), 'a' + rnd(3));
        if (rnd(2)) bits[r / 8] |= (uint8_t)(1 << (r % 8));
        if (rnd(10)) valid[r / 8] |= (uint8_t)(1 << (r % 8));
    }
    offs[n] = (int32_t)bytes.size();
    dfmi_column cols[kCols];
    memset(cols, 0, sizeof cols);
    const void* vals[kCols] = {vi.data(), vf.data(), vi32.data(), vf32.data(), bytes.data(), bits.data(), vu8.data()};
    for (int c = 0; c < kCols; ++c) {
        cols[c].type = kTypes[c];
        cols[c].length = n;
        cols[c].values = vals[c];
        cols[c].validity = c % 2 ? valid.data() : nullptr;
        cols[c].null_count = c % 2 ? 30 : 0;
        cols[c].offsets = kTypes[c] == DFMI_TYPE_UTF8 ? offs.data() : nullptr;
    }
    dfmi_batch batch = {kCols, 0, n, cols};
    int compiled = 0;
    for (int it = 0; it < 3000; ++it) {
        std::vector<dfmi_expr_node> nodes;
        std::vector<std::string> strs;
        strs.reserve(64);
        gen(nodes, 1 + rnd(4), strs);
        const uint32_t flags = (uint32_t)rnd(32);
        dfmi_program* prog = nullptr;
        dfmi_error err;
        if (dfmi_compile_scalar_expr(nodes.data(), (int32_t)nodes.size(), &schema, flags, &prog, &err) == DFMI_OK) {
            ++compiled;
            (void)dfmi_program_name(prog);
            dfmi_program_free(prog);
        }
        char name[256];
        int32_t type = 0;
        (void)oracle_compile_info(nodes.data(), (int32_t)nodes.size(), &schema, flags, name, sizeof name, &type, &err);
        // the oracle evaluates it as a predicate and as a projection
        const dfmi_expr_node* pn[1] = {nodes.data()};
        const int32_t pl[1] = {(int32_t)nodes.size()};
        oracle_result* res = nullptr;
        if (oracle_filter_project(nodes.data(), (int32_t)nodes.size(), pn, pl, 1, &schema, &batch, flags, &res, &err) ==
            DFMI_OK)
            oracle_result_free(res);
        res = nullptr;
        if (oracle_filter_project(nullptr, 0, pn, pl, 1, &schema, &batch, flags, &res, &err) == DFMI_OK) {
            dfmi_column v;
            const char* nm = nullptr;
            for (int i = 0; i < oracle_result_num_columns(res); ++i) oracle_result_column(res, i, &v, &nm);
            oracle_result_free(res);
        }
    }
    printf("expressions: 3000 generated, %d compiled\n", compiled);
    return 0;
}

std::string cell(int t) {
    if (rnd(12) == 0) return "";
    if (rnd(200) == 0) return "x?";  // a parse error now and then
    switch (t) {
        case DFMI_TYPE_UTF8: {
            std::string s;
            for (int i = rnd(8); i > 0; --i) s += "ab,\"x\n"[rnd(6)];
            if (s.find_first_of(",\"\n") != std::string::npos || rnd(4) == 0) {
                std::string q = "\"";
                for (char ch : s) q += ch == '"' ? std::string("\"\"") : std::string(1, ch);
                return q + "\"";
            }
            return s;
        }
        case DFMI_TYPE_BOOLEAN: return rnd(2) ? "true" : "FALSE";
        case DFMI_TYPE_FLOAT64: case DFMI_TYPE_FLOAT32: return std::to_string((double)(int64_t)rng() / 1e9);
        case DFMI_TYPE_UINT8: return std::to_string(rnd(256));
        default: return std::to_string((int32_t)rng());
    }
}

int check_csv() {
    dfmi_field fields[kCols];
    const char* names[kCols] = {"i", "f", "i32", "f32", "s", "b", "u8"};
    for (int c = 0; c < kCols; ++c) fields[c] = {names[c], kTypes[c], 1};
    dfmi_schema schema = {kCols, 0, fields};
    long batches = 0, errors = 0;
    for (int file = 0; file < 12; ++file) {
        char path[64];
        snprintf(path, sizeof path, "/tmp/dfmi_sanitize_%d.csv", file);
        FILE* f = fopen(path, "wb");
        if (!f) return 1;
        const int rows = 1 + rnd(3000);
        const char* nl = file % 2 ? "\r\n" : "\n";
        for (int r = 0; r < rows; ++r) {
            int nc = rnd(30) ? kCols : 1 + rnd(kCols);  // missing trailing fields
            for (int c = 0; c < nc; ++c) fprintf(f, "%s%s", c ? "," : "", cell(kTypes[c]).c_str());
            fputs(rnd(40) ? nl : "", f);  // sometimes no terminator (last line / joined line)
            if (rnd(50) == 0) fputs(nl, f);  // empty record
        }
        fclose(f);
        for (int bs : {1, 3, 64, 1000}) {
            for (int th : {1, 3}) {
                dfmi_csv_reader* R = nullptr;
                dfmi_error err;
                if (dfmi_csv_open(path, &schema, file % 3 == 0, bs, th, &R, &err) != DFMI_OK) return 2;
                while (true) {
                    dfmi_batch b;
                    int32_t has = 0;
                    if (dfmi_csv_next(R, &b, &has, &err) != DFMI_OK) {
                        ++errors;
                        break;
                    }
                    if (!has) break;
                    ++batches;
                    volatile uint64_t acc = 0;  // touch every buffer the batch exposes
                    for (int c = 0; c < b.num_columns; ++c) {
                        const dfmi_column& col = b.columns[c];
                        if (col.type == DFMI_TYPE_UTF8) {
                            for (int64_t r = 0; r <= col.length; ++r) acc += (uint64_t)col.offsets[r];
                            for (int32_t i = 0; i < col.offsets[col.length]; ++i) acc += ((const uint8_t*)col.values)[i];
                        } else if (col.type == DFMI_TYPE_BOOLEAN) {
                            for (int64_t i = 0; i < (col.length + 7) / 8; ++i) acc += ((const uint8_t*)col.values)[i];
                        } else {
                            const int w = col.type == DFMI_TYPE_UINT8 ? 1 : (col.type == DFMI_TYPE_INT32 || col.type == DFMI_TYPE_FLOAT32 ? 4 : 8);
                            for (int64_t i = 0; i < col.length * w; ++i) acc += ((const uint8_t*)col.values)[i];
                        }
                        if (col.validity)
                            for (int64_t i = 0; i < (col.length + 7) / 8; ++i) acc += col.validity[i];
                    }
                }
                dfmi_csv_close(R);
            }
        }
        remove(path);
    }
    printf("csv: %ld batches read, %ld parse errors raised\n", batches, errors);
    return 0;
}

// ---- the aggregate extension's host-only code (csrc/agg_host.cpp)
using dfmi::aggh::GroupMap;
using dfmi::aggh::HKey;
using dfmi::aggh::KeyPart;
using dfmi::aggh::Partial;

// The aggregate table: 7 key columns, then 4 argument columns, all nullable.
constexpr int kKeyCols = 7, kArgCols = 4, kAggCols = kKeyCols + kArgCols;
const int kAggTypes[kAggCols] = {DFMI_TYPE_BOOLEAN, DFMI_TYPE_INT8,    DFMI_TYPE_INT64,  DFMI_TYPE_UINT64,
                                 DFMI_TYPE_FLOAT32, DFMI_TYPE_FLOAT64, DFMI_TYPE_UTF8,   DFMI_TYPE_INT32,
                                 DFMI_TYPE_UINT64,  DFMI_TYPE_FLOAT32, DFMI_TYPE_FLOAT64};
const char* const kAggNames[kAggCols] = {"kb", "k8", "k64", "ku64", "kf32", "kf64", "ks", "a32", "au64", "af32", "af64"};

struct AggTable {
    int n = 0;
    std::vector<uint8_t> kb, valid[kAggCols];
    std::vector<int8_t> k8;
    std::vector<int64_t> k64;
    std::vector<uint64_t> ku64, au64;
    std::vector<float> kf32, af32;
    std::vector<double> kf64, af64;
    std::vector<int32_t> a32, offs;
    std::string bytes;
    int64_t nulls[kAggCols] = {};
    dfmi_column cols[kAggCols];
    const void* values(int c) const {
        const void* v[kAggCols] = {kb.data(),   k8.data(),  k64.data(), ku64.data(), kf32.data(), kf64.data(),
                                   bytes.data(), a32.data(), au64.data(), af32.data(), af64.data()};
        return v[c];
    }
    bool is_valid(int c, int r) const { return (valid[c][r / 8] >> (r % 8)) & 1; }
};

// Keys from small domains (many rows per group) with the edge values: float
// keys one group per bit pattern (NaN, -0.0 / 0.0, inf), Utf8 keys with the
// empty string and strings over 32 bytes. Arguments: NaN, +-inf, -0.0,
// subnormals, and pairs that cancel exactly (1e308, -1e308, 1e-308).
void fill_agg_table(AggTable& t, int n, bool nonfinite) {
    const double kf[] = {0.0, -0.0, 1.5, -2.25, NAN, -NAN, INFINITY, -INFINITY, 5e-324};
    const double af[] = {1e308, -1e308, 1e-308, -1e-308, 5e-324, -5e-324, 0.0, -0.0, 0.1, 3.0, -7.5e-300, 1.7e308};
    const float af4[] = {3e38f, -3e38f, 1e-45f, -1e-45f, 0.0f, -0.0f, 0.1f, 3.0f, 1e-38f, -2.5f};
    const double bad[] = {NAN, INFINITY, -INFINITY};
    const std::string ks[] = {"", "a", "ab", "b", std::string(40, 'x'), std::string(33, 'x') + "y",
                              std::string(33, 'x') + "z"};
    t.n = n;
    const size_t vb = (size_t)(n + 63) / 64 * 8;
    t.kb.assign(vb, 0);
    for (auto& v : t.valid) v.assign(vb, 0);
    t.k8.resize(n), t.k64.resize(n), t.ku64.resize(n), t.kf32.resize(n), t.kf64.resize(n);
    t.a32.resize(n), t.au64.resize(n), t.af32.resize(n), t.af64.resize(n), t.offs.resize(n + 1);
    t.bytes.clear();
    for (int r = 0; r < n; ++r) {
        if (rnd(2)) t.kb[r / 8] |= (uint8_t)(1 << (r % 8));
        t.k8[r] = (int8_t)(rnd(8) ? rnd(4) - 2 : (rnd(2) ? -128 : 127));
        t.k64[r] = rnd(8) ? (int64_t)rnd(5) - 2 : (rnd(2) ? INT64_MIN : INT64_MAX);
        t.ku64[r] = rnd(8) ? (uint64_t)rnd(4) : ~0ull - (uint64_t)rnd(2);
        t.kf64[r] = kf[rnd(9)];
        t.kf32[r] = (float)kf[rnd(8)];
        t.offs[r] = (int32_t)t.bytes.size();
        t.bytes += ks[rnd(7)];
        t.a32[r] = rnd(6) ? (int32_t)rng() : (rnd(2) ? INT32_MIN : INT32_MAX);
        t.au64[r] = rnd(6) ? rng() >> rnd(64) : ~0ull;
        t.af64[r] = nonfinite && rnd(25) == 0 ? bad[rnd(3)] : (rnd(4) ? af[rnd(12)] : (double)(int64_t)rng() / 1e6);
        t.af32[r] = nonfinite && rnd(25) == 0 ? (float)bad[rnd(3)] : (rnd(4) ? af4[rnd(10)] : (float)(int32_t)rng());
        for (int c = 0; c < kAggCols; ++c)
            if (rnd(7)) t.valid[c][r / 8] |= (uint8_t)(1 << (r % 8));
    }
    t.offs[n] = (int32_t)t.bytes.size();
    memset(t.cols, 0, sizeof t.cols);
    for (int c = 0; c < kAggCols; ++c) {
        t.nulls[c] = 0;
        for (int r = 0; r < n; ++r) t.nulls[c] += !t.is_valid(c, r);
        t.cols[c].type = kAggTypes[c];
        t.cols[c].length = n;
        t.cols[c].values = t.values(c);
        t.cols[c].validity = t.valid[c].data();
        t.cols[c].null_count = t.nulls[c];
        t.cols[c].offsets = kAggTypes[c] == DFMI_TYPE_UTF8 ? t.offs.data() : nullptr;
    }
}

// Row r's key part of column c, as the host merge of a batch builds it
// (fixed-width keys: the value bits, integers sign / zero-extended).
KeyPart key_part_of(const AggTable& t, int c, int r) {
    KeyPart k;
    if (!t.is_valid(c, r)) {
        k.null = true;
        return k;
    }
    uint64_t bits = 0;
    switch (kAggTypes[c]) {
        case DFMI_TYPE_UTF8: k.s.assign(t.bytes, (size_t)t.offs[r], (size_t)(t.offs[r + 1] - t.offs[r])); return k;
        case DFMI_TYPE_BOOLEAN: bits = (t.kb[r / 8] >> (r % 8)) & 1; break;
        case DFMI_TYPE_INT8: bits = (uint64_t)(int64_t)t.k8[r]; break;
        case DFMI_TYPE_INT64: bits = (uint64_t)t.k64[r]; break;
        case DFMI_TYPE_UINT64: bits = t.ku64[r]; break;
        case DFMI_TYPE_FLOAT32: {
            uint32_t b;
            memcpy(&b, &t.kf32[r], 4);
            bits = b;
            break;
        }
        default: memcpy(&bits, &t.kf64[r], 8);
    }
    return dfmi::aggh::fixed_part(kAggTypes[c], bits);
}

bool same_value(const dfmi_agg_value& a, const dfmi_agg_value& b) {
    return a.type == b.type && a.is_null == b.is_null && a.count == b.count && a.bits == b.bits;
}

int check_aggregates() {
    dfmi_field fields[kAggCols];
    for (int c = 0; c < kAggCols; ++c) fields[c] = {kAggNames[c], kAggTypes[c], 1};
    dfmi_schema schema = {kAggCols, 0, fields};
    const uint32_t flags = DFMI_FLAG_EXT_AGGREGATE;
    const char* fn_names[4] = {"MIN", "MAX", "SUM", "COUNT"};
    dfmi_error err;
    long groups_compared = 0;
    int cases = 0;
    for (uint64_t seed : {11ull, 12ull, 13ull, 14ull, 15ull, 16ull, 17ull, 18ull, 19ull, 20ull, 21ull, 22ull}) {
        rng.seed(seed);
        AggTable t;
        const int rows = 100 + rnd(300);
        fill_agg_table(t, rows, seed % 3 != 0);
        dfmi_batch batch = {kAggCols, 0, rows, t.cols};
        // 1 to 4 distinct key columns; 1 to 6 aggregates over the argument columns
        const int nk = 1 + rnd(4), n = 1 + rnd(6), ranks = 1 + rnd(3);
        std::vector<int> kc;
        while ((int)kc.size() < nk) {
            const int c = rnd(kKeyCols);
            bool have = false;
            for (int x : kc) have |= x == c;
            if (!have) kc.push_back(c);
        }
        std::vector<dfmi_expr_node> knode(nk), anode(n);
        std::vector<const dfmi_expr_node*> kn(nk), an(n);
        std::vector<int32_t> kl(nk, 1), al(n, 1), rtypes(n);
        std::vector<const char*> names(n);
        std::vector<int> ac(n), fn(n);
        std::vector<dfmi_program*> progs(n, nullptr);
        std::vector<dfmi_aggregate*> aggs(n, nullptr);
        for (int p = 0; p < nk; ++p) {
            memset(&knode[p], 0, sizeof(dfmi_expr_node));
            knode[p].kind = DFMI_EXPR_COLUMN;
            knode[p].column = kc[p];
            kn[p] = &knode[p];
        }
        for (int j = 0; j < n; ++j) {
            ac[j] = kKeyCols + rnd(kArgCols);
            fn[j] = rnd(4);
            names[j] = fn_names[fn[j]];
            rtypes[j] = fn[j] == DFMI_AGG_COUNT ? (int32_t)DFMI_TYPE_UINT64 : kAggTypes[ac[j]];
            memset(&anode[j], 0, sizeof(dfmi_expr_node));
            anode[j].kind = DFMI_EXPR_COLUMN;
            anode[j].column = ac[j];
            an[j] = &anode[j];
            if (dfmi_compile_scalar_expr(&anode[j], 1, &schema, flags, &progs[j], &err) != DFMI_OK) return 10;
            if (dfmi_compile_aggregate(names[j], progs[j], rtypes[j], flags, &aggs[j], &err) != DFMI_OK) return 11;
        }
        // every rank's rows accumulated on the host with the kernels' per-row rules
        std::vector<std::vector<uint8_t>> gpart(ranks), upart(ranks);
        for (int rk = 0; rk < ranks; ++rk) {
            GroupMap groups;
            std::vector<Partial> flat(n);
            for (int r = rk; r < rows; r += ranks) {
                HKey hk;
                for (int p = 0; p < nk; ++p) hk.p.push_back(key_part_of(t, kc[p], r));
                std::vector<Partial>& g = dfmi::aggh::group_entry(groups, std::move(hk), (size_t)n);
                ++g[n].count;
                for (int j = 0; j < n; ++j) {
                    if (!t.is_valid(ac[j], r)) continue;
                    dfmi::aggh::host_accumulate(g[j], fn[j], kAggTypes[ac[j]], (const uint8_t*)t.values(ac[j]), r);
                    dfmi::aggh::host_accumulate(flat[j], fn[j], kAggTypes[ac[j]], (const uint8_t*)t.values(ac[j]), r);
                }
            }
            for (auto& kv : groups)
                for (Partial& q : kv.second) dfmi::aggh::normalize(q);
            for (Partial& q : flat) dfmi::aggh::normalize(q);
            std::vector<int> kt;
            for (int c : kc) kt.push_back(kAggTypes[c]);
            gpart[rk].resize(dfmi::aggh::grouped_bytes(groups, (size_t)n));
            dfmi::aggh::serialize_groups(groups, kt, (size_t)n, gpart[rk].data());
            upart[rk].resize((size_t)n * sizeof(Partial));
            memcpy(upart[rk].data(), flat.data(), upart[rk].size());
        }
        std::vector<const void*> gp(ranks), up(ranks);
        std::vector<int64_t> gsz(ranks);
        for (int rk = 0; rk < ranks; ++rk) {
            gp[rk] = gpart[rk].data();
            up[rk] = upart[rk].data();
            gsz[rk] = (int64_t)gpart[rk].size();
        }
        // grouped: merged partials against the oracle over all rows
        const int64_t cap = rows + 1;
        std::vector<dfmi_agg_value> keys((size_t)cap * dfmi::aggh::layout::kMaxKeys), vals((size_t)cap * n);
        std::vector<dfmi_agg_value> okeys((size_t)cap * nk), ovals((size_t)cap * n);
        int64_t ng = -1, ong = -1;
        if (dfmi_agg_merge_grouped_partials(aggs.data(), n, gp.data(), gsz.data(), ranks, cap, keys.data(), vals.data(), &ng,
                                            &err) != DFMI_OK)
            return 12;
        if (oracle_aggregate_grouped_multi(nullptr, 0, kn.data(), kl.data(), nk, names.data(), an.data(), al.data(),
                                           rtypes.data(), n, &schema, &batch, 0, flags, cap, okeys.data(), ovals.data(),
                                           &ong, -1, nullptr, nullptr, 0, &err) != DFMI_OK)
            return 13;
        if (ng != ong) return 14;
        for (int64_t i = 0; i < ng * nk; ++i)
            if (!same_value(keys[i], okeys[i])) return 15;
        for (int64_t i = 0; i < ng * n; ++i)
            if (!same_value(vals[i], ovals[i])) return 16;
        for (int p = 0; p < nk; ++p) {  // the Utf8 key parts' bytes
            if (kAggTypes[kc[p]] != DFMI_TYPE_UTF8) continue;
            std::vector<int32_t> off((size_t)ng + 1), ooff((size_t)ng + 1);
            std::vector<uint8_t> data(t.bytes.size() + 1), odata(t.bytes.size() + 1);
            int64_t len = -1;
            if (dfmi_agg_merge_grouped_partials_keys_utf8(aggs.data(), n, gp.data(), gsz.data(), ranks, p, off.data(),
                                                          (int64_t)off.size(), data.data(), (int64_t)data.size(), &len,
                                                          &err) != DFMI_OK)
                return 17;
            if (oracle_aggregate_grouped_multi(nullptr, 0, kn.data(), kl.data(), nk, names.data(), an.data(), al.data(),
                                               rtypes.data(), n, &schema, &batch, 0, flags, cap, okeys.data(),
                                               ovals.data(), &ong, p, ooff.data(), odata.data(), (int64_t)odata.size(),
                                               &err) != DFMI_OK)
                return 18;
            if (off != ooff || len != ooff[ng] || memcmp(data.data(), odata.data(), (size_t)len)) return 19;
        }
        groups_compared += ng;
        // ungrouped: the same rows through dfmi_agg_merge_partials
        std::vector<dfmi_agg_value> out(n), oout(n);
        if (dfmi_agg_merge_partials(aggs.data(), n, up.data(), ranks, out.data(), &err) != DFMI_OK) return 20;
        if (oracle_aggregate(nullptr, 0, names.data(), an.data(), al.data(), rtypes.data(), n, &schema, &batch, 0, flags,
                             oout.data(), &err) != DFMI_OK)
            return 21;
        for (int j = 0; j < n; ++j)
            if (!same_value(out[j], oout[j])) return 22;
        for (int j = 0; j < n; ++j) {
            dfmi_aggregate_free(aggs[j]);
            dfmi_program_free(progs[j]);
        }
        ++cases;
    }
    printf("aggregates: %d cases, %ld merged groups bit-identical to the oracle\n", cases, groups_compared);
    return 0;
}

// Every truncation of a valid serialised partial, and every key part's length
// word overwritten with 2^63 and 2^64 - 4, is "bad grouped partial" (each
// attempt from a heap block of exactly the bytes offered).
int check_malformed_partials() {
    dfmi_program prog;
    prog.type = DFMI_TYPE_INT64;
    dfmi_aggregate agg;
    agg.name = "SUM";
    agg.fn = DFMI_AGG_SUM;
    agg.ret_type = DFMI_TYPE_INT64;
    agg.arg = prog;
    const dfmi_aggregate* aggs[1] = {&agg};
    const std::vector<int> kt = {DFMI_TYPE_UTF8, DFMI_TYPE_INT64};
    GroupMap groups;
    for (const char* s : {"", "hello", "a key of more than thirty-two bytes, padded"}) {
        HKey hk;
        hk.p.resize(2);
        hk.p[0].s = s;
        hk.p[1] = dfmi::aggh::fixed_part(DFMI_TYPE_INT64, (uint64_t)strlen(s));
        std::vector<Partial>& g = dfmi::aggh::group_entry(groups, std::move(hk), 1);
        g[0].count = g[1].count = 2;
        g[0].isum = 40 + strlen(s);
    }
    std::vector<uint8_t> good(dfmi::aggh::grouped_bytes(groups, 1));
    dfmi::aggh::serialize_groups(groups, kt, 1, good.data());
    auto rejected = [&](const std::vector<uint8_t>& bytes) {
        const void* parts[1] = {bytes.data()};
        const int64_t sizes[1] = {(int64_t)bytes.size()};
        GroupMap into;
        std::vector<int> types;
        try {
            dfmi::aggh::merge_serialized(into, types, aggs, 1, parts, sizes, 1);
        } catch (const dfmi::Fail& f) {
            return f.code == DFMI_ERR_INVALID_ARGUMENT && f.msg == "bad grouped partial";
        }
        return false;
    };
    if (rejected(good)) return 30;  // (the whole partial merges)
    for (size_t len = 0; len < good.size(); ++len)
        if (!rejected(std::vector<uint8_t>(good.begin(), good.begin() + (ptrdiff_t)len))) return 31;
    // the key parts' length words: header (4 words + kMaxKeys key types), then
    // per group per part {null, bits, length} + the bytes padded to 8, then n + 1 partials
    size_t pos = 8 * (4 + (size_t)dfmi::aggh::layout::kMaxKeys);
    int words = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        for (size_t q = 0; q < kt.size(); ++q) {
            uint64_t len;
            memcpy(&len, &good[pos + 16], 8);
            for (uint64_t bad : {1ull << 63, ~0ull - 3}) {
                std::vector<uint8_t> b = good;
                memcpy(&b[pos + 16], &bad, 8);
                if (!rejected(b)) return 32;
            }
            ++words;
            pos += 24 + (size_t)(len + 7) / 8 * 8;
        }
        pos += 2 * sizeof(Partial);
    }
    if (pos != good.size()) return 33;
    printf("malformed partials: %zu truncations and %d length words rejected\n", good.size(), words);
    return 0;
}

// ---- the host paths' device-free parts (csrc/host_bits.h, host_pool.h, host_plan.cpp)
namespace hst = dfmi::host;

constexpr int64_t kBitN[] = {0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200};

bool bit_at(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }

// append_bits / append_ones at every pos in 0..71 and every n of kBitN, into a
// heap block of exactly ceil((pos + n) / 8) + 8 bytes (the slack append_bits'
// comment promises) pre-filled with random bits: bits below pos kept, bits
// [pos, pos + n) the source's (or ones), and after finish_bitmap the rest of
// the last byte zero -- each against a bit-by-bit loop.
int check_bitmaps() {
    long cases = 0;
    for (int64_t pos = 0; pos <= 71; ++pos)
        for (int64_t n : kBitN) {
            const size_t src_bytes = (size_t)(n + 7) / 8, dst_bytes = (size_t)(pos + n + 7) / 8 + 8;
            std::vector<uint8_t> src(src_bytes), before(dst_bytes);
            for (uint8_t& b : src) b = (uint8_t)rng();
            for (uint8_t& b : before) b = (uint8_t)rng();
            for (int ones = 0; ones < 2; ++ones) {
                std::vector<uint8_t> dst = before;  // (exactly dst_bytes on the heap: ASan sees a byte past it)
                if (ones) hst::append_ones(dst.data(), pos, n);
                else hst::append_bits(dst.data(), pos, src.data(), n);
                for (int64_t i = 0; i < pos; ++i)
                    if (bit_at(dst.data(), i) != bit_at(before.data(), i)) return 40;
                for (int64_t i = 0; i < n; ++i)
                    if (bit_at(dst.data(), pos + i) != (ones ? true : bit_at(src.data(), i))) return 41;
                // (bits past pos + n may be overwritten: the next append, or finish_bitmap, owns them)
                hst::finish_bitmap(dst.data(), pos + n);
                for (int64_t i = 0; i < pos + n; ++i)
                    if (bit_at(dst.data(), i) != (i < pos ? bit_at(before.data(), i) : (ones ? true : bit_at(src.data(), i - pos))))
                        return 43;
                for (int64_t i = pos + n; i < (pos + n + 7) / 8 * 8; ++i)
                    if (bit_at(dst.data(), i)) return 44;
                ++cases;
            }
        }
    printf("bitmaps: %ld append_bits / append_ones / finish_bitmap cases\n", cases);
    return 0;
}

// chunk_rows_for: the chunks tile [0, n) exactly, every chunk but the last is
// a multiple of 512 rows, and a batch up to 1.5 chunks is one chunk.
int check_chunk_rows() {
    unsetenv("DFMI_HOST_CHUNK_ROWS");
    for (int64_t n : {0ll, 1ll, 511ll, 512ll, 513ll, 65536ll, 98304ll, 98305ll, 10000000ll})
        for (double bpr : {0.125, 24.0, 1000.0}) {
            const int64_t crows = hst::chunk_rows_for(n, bpr);
            if (crows < 1) return 50;
            const std::vector<hst::Chunk> ch = hst::chunks_of(n, crows);
            if (ch.empty()) return 51;
            int64_t at = 0;
            for (size_t k = 0; k < ch.size(); ++k) {
                if (ch[k].r0 != at || ch[k].rows < 0 || (n > 0 && ch[k].rows == 0)) return 52;
                if (k + 1 < ch.size() && ch[k].rows % 512) return 53;
                at += ch[k].rows;
            }
            if (at != n) return 54;
            // the target: 48 MiB of input per chunk, 65536 rows at the least
            const int64_t target = std::max<int64_t>((int64_t)(48.0 * (1 << 20) / std::max(bpr, 1.0)), 1 << 16);
            if (n <= target + target / 2 && ch.size() != 1) return 55;
            if (n > target + target / 2 && ch.size() < 2) return 56;
        }
    setenv("DFMI_HOST_CHUNK_ROWS", "512", 1);  // the override: 512-row chunks
    const std::vector<hst::Chunk> ch = hst::chunks_of(2000, hst::chunk_rows_for(2000, 24.0));
    unsetenv("DFMI_HOST_CHUNK_ROWS");
    if (ch.size() != 4 || ch[3].r0 != 1536 || ch[3].rows != 464) return 57;
    printf("chunk rows: 27 cases tile their batches\n");
    return 0;
}

// Half-open byte ranges that must be 256-aligned, disjoint and inside `total`.
struct Regions {
    std::vector<std::pair<size_t, size_t>> r;
    void add(size_t off, size_t bytes) { r.emplace_back(off, off + bytes); }
    bool ok(size_t total) {
        std::sort(r.begin(), r.end());
        for (size_t i = 0; i < r.size(); ++i) {
            if (r[i].first % 256 || r[i].second > total) return false;
            if (i && r[i].first < r[i - 1].second) return false;
        }
        return true;
    }
};

// A batch of Float64, nullable Boolean, Utf8 and Int8 columns (its buffers live in the struct).
struct PlanBatch {
    std::vector<double> f;
    std::vector<uint8_t> bits, valid, data;
    std::vector<int32_t> offs;
    std::vector<int8_t> i8;
    dfmi_column cols[4];
    dfmi_batch batch;
    PlanBatch(int64_t n, bool empty_strings) {
        f.assign((size_t)n, 0.5);
        bits.assign((size_t)(n + 63) / 64 * 8 + 8, 0x5a);
        valid.assign(bits.size(), 0xf7);
        offs.assign((size_t)n + 1, 0);
        for (int64_t r = 0; r < n && !empty_strings; ++r) offs[(size_t)r + 1] = offs[(size_t)r] + (int32_t)(r % 5);
        data.assign((size_t)offs[(size_t)n] + 1, 'x');  // (a zero-length data buffer still has an address)
        i8.assign((size_t)n + 1, 3);
        memset(cols, 0, sizeof cols);
        const int types[4] = {DFMI_TYPE_FLOAT64, DFMI_TYPE_BOOLEAN, DFMI_TYPE_UTF8, DFMI_TYPE_INT8};
        const void* vals[4] = {f.data(), bits.data(), data.data(), i8.data()};
        for (int c = 0; c < 4; ++c) {
            cols[c].type = types[c];
            cols[c].length = n;
            cols[c].values = vals[c];
        }
        if (n == 0) cols[0].values = &cols[0];  // (an empty vector's data() may be null; the pointer is never read)
        cols[1].validity = valid.data();
        cols[1].null_count = n ? 1 : 0;
        cols[2].offsets = offs.data();
        batch = dfmi_batch{4, 0, n, cols};
    }
};

// The fake pin predicate: buffers of at most 200 bytes, and the Int8 column's, count as pinned.
const void* g_direct_base = nullptr;
bool fake_pinned(const void* p, size_t n) { return n <= 200 || p == g_direct_base; }

// The chunk pipeline's input / output plans and hb_layout over batches of 0,
// 1 and 1025 rows with one output of each type: every region 256-aligned,
// disjoint, inside the totals; staged regions one prefix of staged_bytes.
int check_plans() {
    dfmi_field fields[4] = {{"f", DFMI_TYPE_FLOAT64, 0}, {"b", DFMI_TYPE_BOOLEAN, 1}, {"s", DFMI_TYPE_UTF8, 0},
                            {"i", DFMI_TYPE_INT8, 0}};
    dfmi_schema schema = {4, 0, fields};
    const uint32_t flags = DFMI_FLAG_EXT_GATHER_ALL;
    dfmi_program* pred = nullptr;
    dfmi_program* projs[4] = {};
    dfmi_error err;
    dfmi_expr_node nd[3];
    memset(nd, 0, sizeof nd);
    nd[0].kind = DFMI_EXPR_COLUMN, nd[0].column = 0;
    nd[1].kind = DFMI_EXPR_LITERAL, nd[1].data_type = DFMI_TYPE_FLOAT64, nd[1].f64 = 0.25;
    nd[2].kind = DFMI_EXPR_BINARY, nd[2].op = DFMI_OP_GT;
    if (dfmi_compile_scalar_expr(nd, 3, &schema, flags, &pred, &err) != DFMI_OK) return 60;
    for (int c = 0; c < 4; ++c) {
        dfmi_expr_node col;
        memset(&col, 0, sizeof col);
        col.kind = DFMI_EXPR_COLUMN, col.column = c;
        if (dfmi_compile_scalar_expr(&col, 1, &schema, flags, &projs[c], &err) != DFMI_OK) return 61;
    }
    int plans = 0;
    for (int64_t n : {0ll, 1ll, 1025ll})
        for (int empty_strings = 0; empty_strings < 2; ++empty_strings) {
            PlanBatch B(n, empty_strings != 0);
            g_direct_base = B.i8.data();
            const hst::Shape S = hst::call_shape(pred, projs, 4, B.batch);
            if (S.nout != 4 || S.ncols != 4) return 62;
            for (int c = 0; c < 4; ++c)
                if (!S.need[c] || S.otype[c] != B.cols[c].type || S.osrc[c] != c || S.passthrough[c]) return 63;
            // one chunk, and 512-row chunks
            for (int64_t crows : {std::max<int64_t>(n, 1), (int64_t)512}) {
                const std::vector<hst::Chunk> chunks = hst::chunks_of(n, crows);
                std::vector<hst::InPlan> inplans;
                for (const hst::Chunk& ch : chunks) {
                    const hst::InPlan P = hst::plan_chunk_in(B.batch, S.need, ch, fake_pinned);
                    Regions staged, direct;
                    size_t staged_end = 0;
                    for (const hst::Buf& b : P.bufs) {
                        if (!b.src) continue;  // absent
                        if (b.direct != (b.bytes && fake_pinned(b.src, b.bytes))) return 64;
                        (b.direct ? direct : staged).add(b.off, b.bytes + 8);  // (a kernel reads whole words)
                        if (!b.direct) staged_end = std::max(staged_end, b.off + b.bytes);
                    }
                    if (!staged.ok(P.staged_bytes) || staged_end > P.staged_bytes || P.staged_bytes > P.total) return 65;
                    for (auto& r : direct.r)
                        if (r.first < P.staged_bytes) return 66;  // the staged ones are one prefix
                    if (!direct.ok(P.total)) return 67;
                    // values, validity (column b), offsets (column s) of a needed column are planned
                    if (!P.bufs[0].src || !P.bufs[3].src || !P.bufs[4].src || !P.bufs[6].src || !P.bufs[8].src || !P.bufs[9].src)
                        return 68;
                    if (P.bufs[1].src || P.bufs[2].src || P.bufs[5].src) return 69;
                    inplans.push_back(P);
                    ++plans;
                }
                const hst::OutRegion O = hst::plan_chunk_out(S, inplans, std::max<int64_t>(crows, 1));
                Regions out;
                for (int o = 0; o < 4; ++o) {
                    const hst::OutPlan& p = O.col[o];
                    if (S.otype[o] == DFMI_TYPE_UTF8) {
                        out.add(p.offsets, (size_t)(std::max<int64_t>(crows, 1) + 1) * 4);
                        out.add(p.data, p.data_cap + 8);
                        for (const hst::InPlan& P : inplans)
                            if (p.data_cap < P.bufs[6].bytes) return 70;
                    } else {
                        out.add(p.values, p.values_cap + 8);
                        out.add(p.validity, dfmi::bitmap_bytes(std::max<int64_t>(crows, 1)) + 8);
                        if (p.values_cap < (size_t)crows * (size_t)dfmi::type_width(S.otype[o])) return 71;
                    }
                }
                if (!out.ok(O.bytes) || O.bytes % 256 || O.n_bm != 4) return 72;  // Float64, Boolean x 2, Int8
            }
        }
    // hb_layout over the three batches at once
    PlanBatch b0(0, false), b1(1, true), b2(1025, false);
    const dfmi_batch ins[3] = {b0.batch, b1.batch, b2.batch};
    hst::HBLayout Lo;
    hst::hb_layout(pred, projs, 4, ins, 3, Lo);
    Regions in, out;
    for (int b = 0; b < 3; ++b)
        for (int c = 0; c < 4; ++c) {
            const hst::HBLayout::In& L = Lo.lay[(size_t)b * 4 + c];
            const dfmi::ColBytes cb = dfmi::col_bytes(ins[b].columns[c], ins[b].num_rows);
            if (L.nval != cb.values || L.noff != cb.offsets) return 73;
            if (L.nvld != (ins[b].columns[c].null_count > 0 ? cb.validity : 0)) return 74;  // no nulls: not staged
            if (L.nval) in.add(L.val, L.nval);
            if (L.noff) in.add(L.off, L.noff);
            if (L.nvld) in.add(L.vld, L.nvld);
            const hst::HBLayout::Out& O = Lo.olay[(size_t)b * 4 + c];
            const int64_t n = ins[b].num_rows;
            if (c == 2) {
                out.add(O.off, (size_t)(n + 1) * 4);
                out.add(O.dat, std::max<size_t>(O.ndat, 1));
                if (O.ndat != cb.values) return 75;
            } else if (n) {
                out.add(O.val, c == 1 ? dfmi::bitmap_bytes(n) : (size_t)n * (size_t)dfmi::type_width(Lo.otype[c]));
            }
            if (n) out.add(O.vld, dfmi::bitmap_bytes(n));
        }
    if (!in.ok(Lo.in_bytes) || Lo.IB < Lo.in_bytes || Lo.IB % 256) return 76;
    // the outputs' size, which dfmi_host_batches_output_bytes reports, holds every output region
    if (!out.ok(Lo.out_bytes) || Lo.OB < Lo.out_bytes || Lo.OB % 256 || Lo.H < 3 * 256 || Lo.H % 256 || Lo.MB % 256) return 77;
    // ragged / mixed batches are refused with the shared check's texts
    PlanBatch bad(7, false);
    bad.cols[3].length = 6;
    const dfmi_batch two[2] = {b2.batch, bad.batch};
    try {
        hst::hb_layout(pred, projs, 4, two, 2, Lo);
        return 78;
    } catch (const dfmi::Fail& f) {
        if (f.msg != "ragged batch") return 79;
    }
    dfmi_program_free(pred);
    for (dfmi_program* p : projs) dfmi_program_free(p);
    printf("plans: %d chunk plans and one host-batches layout checked\n", plans);
    return 0;
}

// Pool::run with 0, 1 and 1000 tasks at 1 and 4 ways, twice in a row on one
// pool: each task runs exactly once.
int check_pool() {
    for (int ways : {1, 4}) {
        hst::Pool pool(ways - 1);
        if (pool.ways() != ways) return 80;
        for (int round = 0; round < 2; ++round)
            for (int nt : {0, 1, 1000}) {
                std::vector<int> ran((size_t)nt, 0);  // (task i alone writes ran[i])
                hst::Tasks tasks;
                for (int i = 0; i < nt; ++i) tasks.emplace_back([&ran, i] { ++ran[(size_t)i]; });
                pool.run(tasks);
                for (int r : ran)
                    if (r != 1) return 81;
            }
    }
    // the copy tasks: pieces that cover the bytes exactly once
    std::vector<uint8_t> src((size_t)9 << 20), dst(src.size() + 1, 0);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 31 + (i >> 12));
    std::vector<int32_t> off(3 << 18), reb(off.size() + 1, -1);
    for (size_t i = 0; i < off.size(); ++i) off[i] = (int32_t)i;
    hst::Pool pool(3);
    hst::Tasks tasks;
    hst::add_copy(tasks, dst.data(), src.data(), src.size(), pool.ways());
    hst::add_copy_rebase(tasks, reb.data(), off.data(), off.size(), 1000, pool.ways());
    if (tasks.size() < 2) return 82;
    pool.run(tasks);
    if (memcmp(dst.data(), src.data(), src.size()) || dst[src.size()] != 0) return 83;
    for (size_t i = 0; i < off.size(); ++i)
        if (reb[i] != (int32_t)i + 1000) return 84;
    if (reb[off.size()] != -1) return 85;
    printf("pool: every task ran once\n");
    return 0;
}

}  // namespace

int main() {
    if (int rc = check_expressions()) return rc;
    if (int rc = check_csv()) return rc;
    if (int rc = check_aggregates()) return rc;
    if (int rc = check_malformed_partials()) return rc;
    if (int rc = check_bitmaps()) return rc;
    if (int rc = check_chunk_rows()) return rc;
    if (int rc = check_plans()) return rc;
    if (int rc = check_pool()) return rc;
    printf("sanitize driver: clean\n");
    return 0;
}
