// Host-code sanitizer driver (TEST INFRASTRUCTURE): the library's host-only
// front ends -- the expression compiler (csrc/compile.cpp) and the CSV
// reader (csrc/csv_reader.cpp) and the aggregate extension's host-only part
// (csrc/agg_host.cpp: exact-sum arithmetic, the host group map, the partials
// that ranks exchange) -- plus the CPU oracle, built with
// AddressSanitizer + UndefinedBehaviorSanitizer and driven over random
// expressions, random batches, generated CSV files (quotes, CRLF, empty
// and missing fields, bad numbers), random aggregates merged from serialised
// partials and compared bit for bit with the oracle, and malformed partials.
// Exit 0 = no finding; the sanitizers abort on the first one. Built and run
// by tests/test_sanitize_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../datafusion_amd/csrc/agg_host.h"
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

}  // namespace

int main() {
    if (int rc = check_expressions()) return rc;
    if (int rc = check_csv()) return rc;
    if (int rc = check_aggregates()) return rc;
    if (int rc = check_malformed_partials()) return rc;
    printf("sanitize driver: clean\n");
    return 0;
}
