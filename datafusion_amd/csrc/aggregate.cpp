// Aggregate extension (DFMI_FLAG_EXT_AGGREGATE): host side of the fused
// Selection + Aggregate pass with no GROUP BY.
//
// The reference plans `SELECT SUM(e), ... FROM t [WHERE p]` as
// Aggregate(Selection?(TableScan)) (sqlplanner.rs:91-117), compiles each
// AggregateFunction with compile_expr (expression.rs:81-116) and then stops:
// ExecutionContext::execute has no Aggregate arm (context.rs:161
// `unimplemented!()`). Here every input batch is one launch of a
// query-compiled kernel (jit_kernels.cpp generate_agg): predicate, argument and
// reduction fused, partials accumulated in device memory across batches; the
// host merges the accumulator copies exactly and rounds once at the end.
//
// This file: the ungrouped and key-window path and the entry points. The
// arithmetic, the host group map and the partials' wire format are
// agg_host.cpp (no device in it); the device hash table's driver is
// agg_hash.cpp; the coalesced entry points (many batches per call) are
// agg_batches.cpp; the state they share is agg_state.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "agg_state.h"
#include "launch_args.h"
#include "slice.h"

using namespace dfmi;
using namespace dfmi::xi;
using namespace dfmi::aggh;
using namespace dfmi::agg;

namespace dfmi {
namespace agg {

// Static errors, slots and tile shape of one aggregate batch (AggBuilt,
// agg_state.h: the filtered form of exec_plan.cpp's build_plan, over the same
// pieces, exec_internal.h: FilterRelation::next, then each argument over the
// filtered batch in aggregate order).
void build_agg_plan(const dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in, uint32_t flags,
                    const AggDiag& diag, AggBuilt& B, bool low_sel) {
    Err& se = B.se;
    jit::Launch& X = B.X;
    if (pred) check_schema(pred, in);
    if (st->grouped) check_schema(&st->key, in);
    for (const dfmi_aggregate* a : st->aggs) check_schema(&a->arg, in);
    check_not_ragged(in);
    int base = offer_filter_errors(pred, in, flags, se), nf = 0;
    if (st->grouped) {  // the group key is evaluated before the aggregates
        offer_program_errors(&st->key, base, se);
        B.plan.gkey = &st->key;
        B.plan.gkey_ord = base;
        B.plan.gslots = st->gslots;
        base += st->key.length;
    }
    for (const dfmi_aggregate* a : st->aggs) {
        offer_program_errors(&a->arg, base, se);
        jit::AggSpec s;
        s.fn = acc_fn(*a);  // (an AVG accumulates as a SUM, a Utf8 MIN / MAX as a COUNT: the same kernel source and cache key)
        s.prog = &a->arg;
        s.ord_base = base;
        s.arg_type = a->arg.type;
        if (s.fn == DFMI_AGG_SUM && is_float_type(a->arg.type)) s.fslot = nf++;
        B.plan.aggs.push_back(s);
        base += a->arg.length;
    }
    check_ordinal_limit(base);
    if (nf > 4) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: more than 4 floating-point SUMs"};
    B.plan.pred = pred;
    X.in = in;
    Slots slots{X};
    if (pred) slots.prog(pred, X.pred_slots);
    if (st->grouped) slots.prog(&st->key, X.proj_slots);
    for (const dfmi_aggregate* a : st->aggs) slots.prog(&a->arg, X.proj_slots);
    slots.check_limit(kArgCols, kArgUtf8);
    const size_t nload = X.num_cols.size();
    X.BLOCK = 512;
    X.K = nload <= 4 ? 8 : (nload <= 8 ? 4 : 2);
    if (diag.rows_per_thread) X.K = atoi(diag.rows_per_thread);  // diagnostics only
    if (diag.proj_dense) X.proj_dense = atoi(diag.proj_dense) & 1;
    // a predicate that selected < 4% of the rows the last time this state
    // ran the query (dfmi_aggregate_batch keeps the kernel's count): M
    // sub-tiles per block, the arguments loaded by one lane per selected row
    // (jit_kernels.cpp generate_agg; numeric, non-Boolean arguments)
    bool can_sub = pred && !st->grouped && X.utf8_cols.empty();
    for (int s : X.proj_slots) can_sub = can_sub && X.col_type(X.num_cols[s]) != DFMI_TYPE_BOOLEAN;
    for (int s : X.pred_slots) can_sub = can_sub && X.col_type(X.num_cols[s]) != DFMI_TYPE_BOOLEAN;
    // (Q6, same-box A/B profiles/r04/q6_ab.log: M = 1 / 2 / 4 -> 2.88 / 2.57 / 2.54 ms)
    if (can_sub && low_sel && in->num_rows >= (1 << 22)) X.M = 4;
    if (diag.subtiles) X.M = can_sub ? std::max(1, std::min(16, atoi(diag.subtiles))) : 1;  // diagnostics: force M
    if (X.K < 1 || X.K > 32) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad tile shape"};
    B.n_tiles = tiles_of(in->num_rows, (int64_t)X.BLOCK * X.K * X.M);
}

// ... for a batch: a device program limit yields to the static error the
// reference raises first.
void build_batch_plan(const dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in, uint32_t flags,
                      const AggDiag& diag, AggBuilt& B, bool low_sel) {
    static_error_first(B.se, [&] { build_agg_plan(st, pred, in, flags, diag, B, low_sel); });
}

}  // namespace agg
}  // namespace dfmi

namespace {

std::vector<Partial> merge_copies(const dfmi_agg_state* st, const std::vector<uint64_t>& h) {
    const size_t n = st->aggs.size();
    std::vector<Partial> parts(n);
    for (size_t j = 0; j < n; ++j) {
        const bool is_min = st->aggs[j]->fn == DFMI_AGG_MIN;
        for (int c = 0; c < kAggCopies; ++c) merge_into(parts[j], &h[((size_t)c * n + j) * kAggWords], is_min);
        normalize(parts[j]);
    }
    return parts;
}

std::vector<uint64_t> read_acc(dfmi_context* ctx, dfmi_agg_state* st) {
    std::vector<uint64_t> h(st->acc_words);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(h.data(), st->acc.p, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return h;
}

}  // namespace

// GROUP BY: the device window accumulators (win_base / win_width) merged into
// the host's groups, and the device window state reset.
void dfmi::agg::flush_groups(dfmi_context* ctx, dfmi_agg_state* st) {
    if (!st->dirty) return;
    const std::vector<uint64_t> h = read_acc(ctx, st);
    const size_t n = st->aggs.size(), na = n + 1;
    const int kt = st->key.type;
    for (int g = 0; g <= st->win_width; ++g) {
        GroupState parts(na);
        for (size_t j = 0; j < na; ++j) {
            const bool is_min = j < n && st->aggs[j]->fn == DFMI_AGG_MIN;
            for (int c = 0; c < kAggCopies; ++c)
                merge_into(parts[j], &h[(((size_t)c * st->gslots + g) * na + j) * kAggWords], is_min);
            normalize(parts[j]);
        }
        if (parts[n].count == 0) continue;  // no row of this key in the window
        HKey hk;
        if (g == st->win_width) {
            hk.p.emplace_back();
            hk.p.back().null = true;
        } else {
            hk.p.push_back(fixed_part(kt, st->win_base + (uint64_t)g));
        }
        merge_group(group_entry(st->groups, std::move(hk), n), parts, st->aggs.data(), n);
    }
    HIP_TRY(hipMemcpyAsync(st->acc.p, st->init.data(), st->acc_words * 8, hipMemcpyHostToDevice, ctx->stream));
    st->dirty = false;
}

namespace {

// Every group the state holds (window, hash table, host merges) in st->groups.
void collect_groups(dfmi_context* ctx, dfmi_agg_state* st) {
    flush_groups(ctx, st);
    drain_hashed(ctx, st);
    st->shown.reset();
}

// The state's device accumulators: `cells` cells of `na` records, the first
// aggs.size() of a cell its aggregates'. Their zero state (MIN keys all ones)
// stays in st->init for the resets.
void alloc_accumulators(dfmi_context* ctx, dfmi_agg_state* st, size_t cells, size_t na) {
    st->acc_words = cells * na * kAggWords;
    st->init.assign(st->acc_words, 0);
    for (size_t c = 0; c < cells; ++c)
        for (size_t j = 0; j < st->aggs.size(); ++j)
            if (st->aggs[j]->fn == DFMI_AGG_MIN) st->init[(c * na + j) * kAggWords + 2] = ~0ull;
    st->acc.alloc(st->acc_words * 8);
    HIP_TRY(hipMemcpyAsync(st->acc.p, st->init.data(), st->acc_words * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// The test hooks' answer: the kernel a batch of this shape would launch
// (`key`: the GROUP BY form), generated and, if asked, compiled with hipRTC;
// the source's length, its text into buf.
int64_t agg_jit_source(const dfmi_program* pred, const dfmi_program* key, const dfmi_aggregate* const* aggs, int32_t n,
                       const dfmi_batch* in, uint32_t flags, int32_t compile, char* buf, int64_t cap) {
    dfmi_agg_state st;
    if (key) {
        st.grouped = true;
        st.key = *key;
        st.keys.push_back(*key);
        st.gslots = key->type == DFMI_TYPE_BOOLEAN ? 3 : 17;
    }
    for (int j = 0; j < n; ++j) st.aggs.push_back(aggs[j]);
    AggBuilt B;
    build_agg_plan(&st, pred, in, flags & ~0x40000000u, agg_diag(), B);
    if (flags & 0x40000000u) {  // the coalesced-batches form of the kernel (agg_batches.cpp)
        B.X.batched = true;
        B.X.M = 1;
    }
    const std::string src = jit::generate(B.plan, B.X);
    if (compile) (void)jit::compile_code(src, nullptr);
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", src.c_str());
    return (int64_t)src.size();
}

std::vector<int> key_types(const dfmi_agg_state* st) {
    std::vector<int> t;
    for (const dfmi_program& k : st->keys) t.push_back(k.type);
    return t;
}

}  // namespace

// A state under construction: freed with everything it owns unless released.
using StatePtr = std::unique_ptr<dfmi_agg_state, decltype(&dfmi_agg_state_free)>;

extern "C" int32_t dfmi_agg_state_create(dfmi_context* ctx, const dfmi_aggregate* const* aggs, int32_t n,
                                         dfmi_agg_state** out, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !out || n <= 0 || !aggs) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        if (n > 16) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: more than 16 aggregates"};
        StatePtr st(new dfmi_agg_state(), dfmi_agg_state_free);
        st->device = ctx->device;
        for (int j = 0; j < n; ++j) {
            if (!aggs[j]) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL aggregate"};
            st->aggs.push_back(aggs[j]);
        }
        HIP_TRY(hipSetDevice(ctx->device));
        alloc_accumulators(ctx, st.get(), kAggCopies, (size_t)n);
        strext_create(ctx, st.get());
        *out = st.release();
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_agg_state_create_grouped_multi(dfmi_context* ctx, const dfmi_program* const* keys,
                                                       int32_t num_keys, const dfmi_aggregate* const* aggs, int32_t n,
                                                       dfmi_agg_state** out, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !out || !keys || num_keys <= 0 || n <= 0 || !aggs) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        if (num_keys > dfmi::gb::kMaxKeys)
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: more than 4 GROUP BY expressions"};
        for (int p = 0; p < num_keys; ++p) {
            if (!keys[p]) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL key"};
            const int kt = keys[p]->type;
            if (kt != DFMI_TYPE_BOOLEAN && !is_numeric_type(kt) && kt != DFMI_TYPE_UTF8)
                throw Fail{DFMI_ERR_NOT_IMPLEMENTED, std::string("GROUP BY over ") + type_debug(kt)};
        }
        if (n > dfmi::gb::kMaxAggs) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: more than 15 grouped aggregates"};
        StatePtr st(new dfmi_agg_state(), dfmi_agg_state_free);
        st->device = ctx->device;
        st->grouped = true;
        for (int p = 0; p < num_keys; ++p) st->keys.push_back(*keys[p]);
        st->key = *keys[0];
        const int kt = st->key.type;
        for (int j = 0; j < n; ++j) {
            if (!aggs[j]) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL aggregate"};
            st->aggs.push_back(aggs[j]);
        }
        HIP_TRY(hipSetDevice(ctx->device));
        // one Boolean / integer key: the window kernel (16 consecutive values
        // per batch, more through the hash table); anything else: the hash table
        // (a state with a Utf8 MIN / MAX takes no key window: every batch through the hash table, whose
        // passes know each row's dense group id)
        const bool strings = any_utf8_extreme(st->aggs.data(), st->aggs.size());
        if (num_keys == 1 && (kt == DFMI_TYPE_BOOLEAN || !host_keyed(kt)) && !strings) {
            st->gslots = kt == DFMI_TYPE_BOOLEAN ? 3 : 17;  // false, true / 16 consecutive values; + null
            alloc_accumulators(ctx, st.get(), (size_t)kAggCopies * st->gslots, (size_t)n + 1);  // (+ the group's rows)
            if (kt != DFMI_TYPE_BOOLEAN) {
                dfmi_error e2{};
                for (int i = 0; i < 2; ++i)
                    if (dfmi_compile_aggregate(i ? "MAX" : "MIN", keys[0], kt, DFMI_FLAG_EXT_AGGREGATE, &st->mm[i], &e2) !=
                        DFMI_OK)
                        throw Fail{e2.code, e2.message};
                const dfmi_aggregate* mm[2] = {st->mm[0], st->mm[1]};
                if (dfmi_agg_state_create(ctx, mm, 2, &st->mm_state, &e2) != DFMI_OK) throw Fail{e2.code, e2.message};
            }
        }
        strext_create(ctx, st.get());
        *out = st.release();
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_agg_state_create_grouped(dfmi_context* ctx, const dfmi_program* key,
                                                 const dfmi_aggregate* const* aggs, int32_t n, dfmi_agg_state** out,
                                                 dfmi_error* err) {
    if (!key) {
        set_err(err, DFMI_ERR_INVALID_ARGUMENT, "bad argument");
        return DFMI_ERR_INVALID_ARGUMENT;
    }
    const dfmi_program* keys[1] = {key};
    return dfmi_agg_state_create_grouped_multi(ctx, keys, 1, aggs, n, out, err);
}

extern "C" int32_t dfmi_agg_state_num_keys(const dfmi_agg_state* st) {
    return st && st->grouped ? (int32_t)st->keys.size() : 0;
}

extern "C" int32_t dfmi_agg_state_finish_grouped(dfmi_context* ctx, dfmi_agg_state* st, int64_t cap,
                                                 dfmi_agg_value* keys, dfmi_agg_value* values, int64_t* num_groups,
                                                 dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || !num_groups) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (!st->grouped) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "not a GROUP BY state"};
        check_not_failed(st);
        const AggDiag diag = agg_diag();
        HIP_TRY(hipSetDevice(ctx->device));
        flush_groups(ctx, st);  // the key window's rows into the host's groups, whichever finish follows
        {
            const auto t0 = std::chrono::steady_clock::now();
            if (finish_device(ctx, st, diag, cap, keys, values, num_groups)) {
                if (diag.finish_profile)
                    fprintf(stderr, "[dfmi finish] %lld groups on the device: %.1f us\n", (long long)*num_groups,
                            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
                return DFMI_OK;
            }
        }
        if (finish_flat(ctx, st, diag)) {
            const auto t0 = std::chrono::steady_clock::now();
            emit_flat(st, *st->flat, cap, keys, values, num_groups);
            if (st->sx) st->sx->finished = true;  // (the values exist: dfmi_agg_state_value_bytes may be asked)
            if (diag.finish_profile)
                fprintf(stderr, "[dfmi finish] emit %.1f us\n",
                        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            return DFMI_OK;
        }
        collect_groups(ctx, st);
        emit_groups(st->groups, key_types(st), st->aggs.data(), st->aggs.size(), cap, keys, values, num_groups);
        if (st->sx) st->sx->finished = true;
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_agg_state_group_keys_utf8_part(const dfmi_agg_state* st, int32_t part, int32_t* offsets,
                                                       int64_t num_offsets, uint8_t* data, int64_t data_capacity,
                                                       int64_t* data_length, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!st || !data_length) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        check_not_failed(st);
        if (!st->grouped || part < 0 || part >= (int32_t)st->keys.size() || st->keys[part].type != DFMI_TYPE_UTF8)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "not a GROUP BY state over a Utf8 key"};
        if (!st->shown && st->flat)
            emit_key_bytes_flat(*st->flat, part, offsets, num_offsets, data, data_capacity, data_length);
        else
            emit_key_bytes(st->shown ? *st->shown : st->groups, part, offsets, num_offsets, data, data_capacity,
                           data_length);
        return DFMI_OK;
    });
}

// The values of Utf8 MIN / MAX aggregate `agg` from the state's last finish, in its order.
extern "C" int32_t dfmi_agg_state_value_bytes(const dfmi_agg_state* st, int32_t agg, int32_t* offsets,
                                              int64_t num_offsets, uint8_t* data, int64_t data_capacity,
                                              int64_t* data_length, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!st || !data_length) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        *data_length = 0;
        check_not_failed(st);
        if (agg < 0 || agg >= (int32_t)st->aggs.size() || !is_utf8_extreme(*st->aggs[agg]) || !st->sx)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "not a Utf8 MIN / MAX aggregate of this state"};
        if (!st->sx->finished) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "no finish yet"};
        if (!st->grouped) {
            emit_value_bytes(std::vector<StrVal>{st->sx->one[(size_t)agg]}, offsets, num_offsets, data, data_capacity, data_length);
        } else if (!st->shown && st->flat) {
            const FlatGroups& f = *st->flat;
            size_t x = 0;
            while (st->sx->x[x].agg != agg) ++x;
            std::vector<StrVal> vals((size_t)f.ng);  // (a group without a counted row has no persisted winner: null)
            for (uint64_t i = 0; i < f.ng; ++i) vals[i] = strext_flat_value(f, x, f.order[i]);
            emit_value_bytes(vals, offsets, num_offsets, data, data_capacity, data_length);
        } else {
            emit_value_bytes(st->groups, agg, offsets, num_offsets, data, data_capacity, data_length);
        }
        return DFMI_OK;
    });
}

// Internal test hook (not part of the C ABI, not declared in include/): the bytes reserved for the string
// arena of a state's Utf8 MIN / MAX aggregates (0: none).
extern "C" long long dfmi_internal_agg_str_arena_bytes(const dfmi_agg_state* st) {
    return st && st->sx ? (long long)st->sx->arena_cap : 0;
}

extern "C" int32_t dfmi_agg_state_group_keys_utf8(const dfmi_agg_state* st, int32_t* offsets, int64_t num_offsets,
                                                  uint8_t* data, int64_t data_capacity, int64_t* data_length,
                                                  dfmi_error* err) {
    return dfmi_agg_state_group_keys_utf8_part(st, 0, offsets, num_offsets, data, data_capacity, data_length, err);
}

extern "C" int32_t dfmi_agg_state_reset(dfmi_context* ctx, dfmi_agg_state* st, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        HIP_TRY(hipSetDevice(ctx->device));
        if (st->acc.p)
            HIP_TRY(hipMemcpyAsync(st->acc.p, st->init.data(), st->acc_words * 8, hipMemcpyHostToDevice, ctx->stream));
        const AggDiag diag = agg_diag();
        if (st->hd) reset_table(ctx, *st->hd, diag);
        strext_reset(ctx, st, diag);
        if (st->sx) {  // (and no finish to ask dfmi_agg_state_value_bytes about)
            st->sx->finished = false;
            st->sx->one.assign(st->aggs.size(), StrVal{});
        }
        st->failed = false;
        st->failure = dfmi_error{};
        st->index.clear();
        st->groups.clear();
        if (st->flat) st->spare_flat = std::move(st->flat);
        st->shown.reset();
        st->win_width = -1;
        st->dirty = false;
        if (st->mm_state) {
            dfmi_error e2{};
            if (dfmi_agg_state_reset(ctx, st->mm_state, &e2) != DFMI_OK) throw Fail{e2.code, e2.message};
        }
        return DFMI_OK;
    });
}

extern "C" void dfmi_agg_state_free(dfmi_agg_state* st) {
    if (!st) return;
    dfmi_agg_state_free(st->mm_state);
    dfmi_aggregate_free(st->mm[0]);
    dfmi_aggregate_free(st->mm[1]);
    (void)hipSetDevice(st->device);
    delete st;  // (with the device memory it owns)
}

extern "C" int32_t dfmi_aggregate_batch(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred,
                                        const dfmi_batch* in, uint32_t flags, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || !in || (in->num_columns > 0 && !in->columns))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        check_not_failed(st);
        const AggDiag diag = agg_diag();
        if (st->grouped) unflatten(st);  // a finish's flat groups back in the map before more rows merge
        Unsliced us_;  // sliced arrays (arrow offsets): offset-0 views / shifted bitmaps (slice.cpp)
        if (any_offset(in, 1)) {
            HIP_TRY(hipSetDevice(ctx->device));
            in = unslice(in, 1, us_, true, ctx->stream);
        }
        if (st->grouped && (!st->acc.p || diag.group_host)) {
            // several keys, a float or Utf8 key: the keys and the arguments
            // through one fused Selection + Projection pass, then the device
            // hash table (or, diagnostics, the host merge)
            HIP_TRY(hipSetDevice(ctx->device));
            if (in->num_rows > 0) {
                if (st->acc.p) flush_groups(ctx, st);
                if (diag.group_host) group_batch_on_host(ctx, st, pred, in, flags);
                else group_batch_hashed(ctx, st, pred, in, flags, diag);
            }
            return DFMI_OK;
        }
        // the query's selectivity last time (this state, this predicate)
        const uint64_t hint_key = (uint64_t)(uintptr_t)st * 1099511628211ull ^ (uint64_t)(uintptr_t)pred;
        const auto hint = ctx->sel_hint.find(hint_key);
        const bool low_sel = hint != ctx->sel_hint.end() && hint->second < 0.04;
        AggBuilt B;
        build_batch_plan(st, pred, in, flags, diag, B, low_sel);
        Err& se = B.se;
        const int64_t n = in->num_rows;
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t stream = ctx->stream;
        if (st->grouped && n > 0) {
            // the batch's key window: Boolean keys always [false, true];
            // integer keys 16 values from the batch's smallest selected key
            uint64_t wbase = 0;
            int wwidth = 2;
            if (st->key.type != DFMI_TYPE_BOOLEAN) {
                wwidth = st->gslots - 1;
                dfmi_error e2{};
                dfmi_agg_value mm[2];
                if (dfmi_aggregate_batch(ctx, st->mm_state, pred, in, flags, &e2) != DFMI_OK ||
                    dfmi_agg_state_finish(ctx, st->mm_state, mm, &e2) != DFMI_OK ||
                    dfmi_agg_state_reset(ctx, st->mm_state, &e2) != DFMI_OK) {
                    // the predicate or the key failed: evaluated before any aggregate
                    st->failed = true;
                    st->failure = e2;
                    throw Fail{e2.code, e2.message};
                }
                const bool cover = st->win_width == wwidth && (mm[0].count == 0 || ((mm[0].bits - st->win_base) < (uint64_t)wwidth &&
                                                                                   (mm[1].bits - st->win_base) < (uint64_t)wwidth));
                if (cover) {
                    wbase = st->win_base;
                } else {
                    wbase = mm[0].count ? mm[0].bits : 0;
                    if (mm[0].count && mm[1].bits - mm[0].bits >= (uint64_t)wwidth) {
                        // wider than the device window: the hash table (its
                        // fused pass raises the same first error in the same
                        // evaluation order as the grouped kernel would)
                        flush_groups(ctx, st);
                        group_batch_hashed(ctx, st, pred, in, flags, diag);
                        return DFMI_OK;
                    }
                }
            }
            if (st->win_width != wwidth || st->win_base != wbase) {
                flush_groups(ctx, st);
                st->win_base = wbase;
                st->win_width = wwidth;
            }
        }
        ctx->timed = false;
        ctx->last_compile_ms = 0;
        uint64_t dev_key = ~0ull;
        int dev_kind = 0;
        if (n > 0) {
            jit::Launch& X = B.X;
            const hipFunction_t fn = query_kernel(ctx, B.plan, X, se);
            Args A;
            memset(&A, 0, sizeof A);
            A.n_rows = n;
            A.n_tiles = (int)B.n_tiles;
            bind_inputs(A, X, in);
            bind_literals(A, X);
            const WsLease ws = ws_acquire(ctx, 0, stream);
            bind_workspace(A, ws);
            A.agg = st->acc.as<unsigned long long>();
            A.gbase = st->win_base;
            A.gwidth = st->win_width;
            HIP_TRY(hipEventRecord(ctx->ev0, stream));
            launch_query(fn, (unsigned)B.n_tiles, X.BLOCK, A, stream);
            count_query_launch();
            ws_commit(ctx, ws);
            HIP_TRY(hipEventRecord(ctx->ev1, stream));
            HIP_TRY(hipMemcpyAsync(ctx->host_hdr.p, ws.hdr, kHdrAlloc, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipEventRecord(ctx->ev2, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            uint64_t ew;
            memcpy(&ew, ctx->host_hdr.p + kHdrErr, 8);
            if (pred && !st->grouped) {  // the kernel's count of selected rows in every 64th block
                uint64_t sel;
                memcpy(&sel, ctx->host_hdr.p + kHdrTotals, 8);
                const int64_t tile_rows = (int64_t)X.BLOCK * X.K * X.M;
                int64_t sampled = 0;
                for (int64_t b = 0; b < B.n_tiles; b += 64) sampled += std::min(tile_rows, n - b * tile_rows);
                ctx->sel_hint[hint_key] = sampled ? (double)sel / (double)sampled : 1.0;
            }
            decode_err_word(ew, dev_key, dev_kind);
            read_timing(ctx, true);
        }
        if (st->grouped && n > 0) st->dirty = true;
        Fail fail{DFMI_OK, ""};
        if (dev_kind == ERRK_CAPACITY)  // a key outside the window the pre-pass found: cannot happen
            fail = Fail{DFMI_ERR_DEVICE, "GROUP BY key outside the batch's key window"};
        else if (dev_kind && (!se.set || dev_key < se.key))
            fail = device_fail(dev_kind);
        else if (se.set)
            fail = Fail{se.code, se.msg};
        if (fail.code != DFMI_OK) {
            // the query has failed (the state holds partial sums of this batch)
            st->failed = true;
            set_err(&st->failure, fail.code, fail.msg);
            throw fail;
        }
        // Utf8 MIN / MAX (ungrouped; in the kernel above they counted): the string passes
        // (the records have counted the batch: a failure here fails the query like the kernel's own)
        if (!st->grouped && st->sx && n > 0) {
            try {
                strext_batch_ungrouped(ctx, st, pred, in, flags, diag);
            } catch (const Fail& f) {
                st->failed = true;
                set_err(&st->failure, f.code, f.msg);
                throw;
            }
        }
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_agg_state_finish(dfmi_context* ctx, dfmi_agg_state* st, dfmi_agg_value* out,
                                         dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || !out) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        check_not_failed(st);
        if (st->grouped) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "a GROUP BY state: dfmi_agg_state_finish_grouped"};
        const std::vector<Partial> parts = merge_copies(st, read_acc(ctx, st));
        for (size_t j = 0; j < st->aggs.size(); ++j) out[j] = finish_one(*st->aggs[j], parts[j]);
        strext_finish_ungrouped(ctx, st, out);
        return DFMI_OK;
    });
}

extern "C" int64_t dfmi_agg_partial_bytes(const dfmi_agg_state* st) {
    return st ? (int64_t)(st->aggs.size() * sizeof(Partial)) : 0;
}

extern "C" int32_t dfmi_agg_state_partial(dfmi_context* ctx, dfmi_agg_state* st, void* host_out, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || !host_out) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        check_not_failed(st);
        if (st->grouped) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "partial state of a GROUP BY aggregate"};
        if (st->sx) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        const std::vector<Partial> parts = merge_copies(st, read_acc(ctx, st));
        memcpy(host_out, parts.data(), parts.size() * sizeof(Partial));
        return DFMI_OK;
    });
}

extern "C" int64_t dfmi_agg_state_grouped_partial_bytes(dfmi_context* ctx, dfmi_agg_state* st, dfmi_error* err) {
    return guarded_size(err, [&]() -> int64_t {
        if (!ctx || !st) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (!st->grouped) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "not a GROUP BY state"};
        check_not_failed(st);
        if (st->sx) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        HIP_TRY(hipSetDevice(ctx->device));
        collect_groups(ctx, st);
        return (int64_t)grouped_bytes(st->groups, st->aggs.size());
    });
}

extern "C" int32_t dfmi_agg_state_grouped_partial(dfmi_context* ctx, dfmi_agg_state* st, void* host_out, int64_t bytes,
                                                  dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || !host_out) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (!st->grouped) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "not a GROUP BY state"};
        check_not_failed(st);
        if (st->sx) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        HIP_TRY(hipSetDevice(ctx->device));
        collect_groups(ctx, st);
        if ((size_t)bytes < grouped_bytes(st->groups, st->aggs.size()))
            throw Fail{DFMI_ERR_CAPACITY, "partial buffer too small"};
        serialize_groups(st->groups, key_types(st), st->aggs.size(), (uint8_t*)host_out);
        return DFMI_OK;
    });
}

// dfmi_shard_agg_finish_grouped's merge (shard.cpp): every rank's partials
// merged into the state's shown groups, so the Utf8 key bytes of the merged
// groups come from dfmi_agg_state_group_keys_utf8* afterwards.
int32_t dfmi_agg_state_show_merged(dfmi_agg_state* st, const void* const* partials, const int64_t* sizes, int32_t nparts,
                                   int64_t cap, dfmi_agg_value* keys, dfmi_agg_value* values, int64_t* num_groups,
                                   dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!st || !st->grouped || !partials || !sizes || nparts <= 0 || !num_groups)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        if (st->sx) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, kUtf8ExtremePartial};
        auto merged = std::make_shared<GroupMap>();
        std::vector<int> kt = key_types(st);
        merge_serialized(*merged, kt, st->aggs.data(), st->aggs.size(), partials, sizes, nparts);
        emit_groups(*merged, kt, st->aggs.data(), st->aggs.size(), cap, keys, values, num_groups);
        st->shown = merged;
        return DFMI_OK;
    });
}

// Internal test hook (not part of the C ABI, not declared in include/): the
// aggregate kernel a dfmi_aggregate_batch call would launch, generated and
// (compile != 0) compiled with hipRTC -- no device needed (tests/test_aggregate_cpu.py).
// Flag bit 0x40000000 (as dfmi_internal_jit_check): the batched form a
// dfmi_aggregate_batches call launches (tests/test_agg_batches_cpu.py).
// Diagnostics: grouped batches accumulated by the bucketed passes (groupby.h) in this process.
extern "C" long dfmi_internal_group_bucketed_batches() { return bucketed_batches(); }
// Diagnostics: times the exact-sum digits' normalisation threshold tripped (accumulate_hashed) in this process.
extern "C" long dfmi_internal_group_normalize_trips() { return normalize_trips(); }
// Diagnostics: kernel launches of groupby.hip / str_extreme.hip whose work exceeded one trip of their grid
// (groupby.h "Diagnostic grid cap") in this process.
extern "C" long dfmi_internal_group_strided_launches() { return strided_launches(); }
// Diagnostics: the hash table's device records of groups [g0, g0 + ng), by group id, as they stand (a carry pass
// preserves an exact sum's value, so only the digits themselves show whether it ran over a record): out
// [ng][words] (null: only info), info [3 + 15]: words, groups, float SUMs, their digit offsets.
extern "C" int32_t dfmi_internal_group_records(dfmi_context* ctx, dfmi_agg_state* st, uint64_t g0, uint64_t ng,
                                               uint64_t* out, int64_t* info, dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || !info) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        read_records(ctx, st, g0, ng, out, info);
        return DFMI_OK;
    });
}

extern "C" int64_t dfmi_internal_agg_jit_check(const dfmi_program* pred, const dfmi_aggregate* const* aggs, int32_t n,
                                               const dfmi_batch* in, uint32_t flags, int32_t compile, char* buf,
                                               int64_t cap, dfmi_error* err) {
    return guarded_size(err, [&]() -> int64_t {
        if (!in || !aggs || n <= 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        return agg_jit_source(pred, nullptr, aggs, n, in, flags, compile, buf, cap);
    });
}

// Internal test hook: the GROUP BY form of the above (key: a Boolean or
// integer program).
extern "C" int64_t dfmi_internal_agg_grouped_jit_check(const dfmi_program* pred, const dfmi_program* key,
                                                       const dfmi_aggregate* const* aggs, int32_t n,
                                                       const dfmi_batch* in, uint32_t flags, int32_t compile, char* buf,
                                                       int64_t cap, dfmi_error* err) {
    return guarded_size(err, [&]() -> int64_t {
        if (!in || !aggs || !key || n <= 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        return agg_jit_source(pred, key, aggs, n, in, flags, compile, buf, cap);
    });
}
