// Aggregate extension: the coalesced entry points. Many small batches (the
// reference streams 1024-row batches through Relation::next) accumulated into
// one dfmi_agg_state by one call: one batch table H2D, one launch of the
// batched form of the aggregate kernel (jit_kernels.cpp emit_batched_prologue: a
// block finds its batch through Args::tile_batch and takes its rows, columns
// and error word from its row of Args::batch_ptrs), one D2H of the per-batch
// headers, one synchronisation -- instead of all of that once per batch.
//
// The state afterwards is the state after dfmi_aggregate_batch on the same
// batches in order; the error is the first failing batch's, in order: every
// batch has its own error word (a later batch's error at an earlier ordinal
// must not win over an earlier batch's).
//
// Ungrouped states and the key-window kernel run coalesced; the window is one
// for the whole call (a coalesced MIN / MAX pre-pass). Hash-table states run
// the fused evaluation pass as one coalesced launch into per-batch segments,
// pack them dense (groupby.hip k_group_concat) and run the table's passes
// once over the call's rows (agg_hash.cpp group_batches_hashed). States that
// read Utf8 columns run the call one batch at a time through the same entry
// point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "agg_state.h"
#include "batch_table.h"
#include "launch_args.h"
#include "slice.h"

using namespace dfmi;
using namespace dfmi::xi;
using namespace dfmi::agg;

namespace {

std::atomic<long> g_query_launches{0};

// Packed input bytes one host call stages at a time (larger calls are split at batch boundaries).
constexpr size_t kStageBudget = (size_t)64 << 20;

// A call's first failure: the batch and the error dfmi_aggregate_batch would have raised on it.
struct Failure {
    int32_t batch = -1;
    Fail fail{DFMI_OK, ""};
    bool failed() const { return batch >= 0; }
};

// Batches [0, nb) through ONE launch of st's batched kernel (ungrouped, or
// the key-window kernel over the window gbase / gwidth). The accumulators
// hold partial sums of every batch afterwards, also of those behind the
// first failing one: the caller fails the state.
Failure run_batched(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins, int32_t nb,
                    uint32_t flags, const AggDiag& diag) {
    Failure R;
    if (nb <= 0) return R;
    const ShapeBatch S(ins, nb);
    AggBuilt B;
    build_batch_plan(st, pred, &S.view, flags, diag, B, false);
    jit::Launch& X = B.X;
    X.batched = true;
    X.M = 1;  // (no sub-tiles in the batched form)
    const TileLayout L(ins, nb, (int64_t)X.BLOCK * X.K);
    const int64_t T = L.T;
    BatchTable table(X, S, L, nb, 0);  // (no output slots: the kernel accumulates into the state)
    if (T > 0) {
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t stream = ctx->stream;
        ctx->timed = false;
        ctx->last_compile_ms = 0;
        const hipFunction_t fn = query_kernel(ctx, B.plan, X, B.se);
        table.in_context(ctx);
        table.ones = ensure_ones(ctx, S, ins, nb, stream);
        for (int32_t b = 0; b < nb; ++b) table.write_row(b, ins[b]);
        HIP_TRY(hipMemcpyAsync(table.dev_meta, table.host_meta, table.meta_bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(table.dev_hdr, 0, table.hdr_bytes, stream));
        Args A;
        memset(&A, 0, sizeof A);
        A.n_rows = S.maxn;
        A.n_tiles = (int)T;
        bind_literals(A, X);
        const WsLease ws = ws_acquire(ctx, 0, stream);
        bind_workspace(A, ws);
        A.tile_batch = (const int*)(table.dev_meta + table.table_bytes);
        A.batch_ptrs = (void* const*)table.dev_meta;
        A.agg = st->acc.as<unsigned long long>();
        A.gbase = st->win_base;
        A.gwidth = st->win_width;
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev0, stream));
        launch_query(fn, (unsigned)T, X.BLOCK, A, stream);
        count_query_launch();
        ws_commit(ctx, ws);
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev1, stream));
        HIP_TRY(hipMemcpyAsync(ctx->host_bhdr.p, table.dev_hdr, table.hdr_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (ctx->timing) read_timing(ctx, false);
    }
    // ---- in batch order: the first batch dfmi_aggregate_batch would have failed on
    const Err& se = B.se;
    for (int32_t b = 0; b < nb; ++b) {
        uint64_t dev_key = ~0ull;
        int dev_kind = 0;
        if (table.host_hdr && ins[b].num_rows > 0)
            decode_err_word(batch_hdr(table.host_hdr, b)[kBatchHdrErr], dev_key, dev_kind);
        if (dev_kind == ERRK_CAPACITY) {  // a key outside the window the pre-pass found: cannot happen
            R.batch = b;
            R.fail = Fail{DFMI_ERR_DEVICE, "GROUP BY key outside the batch's key window"};
        } else if (dev_kind && (!se.set || dev_key < se.key)) {
            R.batch = b;
            R.fail = device_fail(dev_kind);
        } else if (se.set) {  // a static error: every batch has it, the first raises it
            R.batch = b;
            R.fail = Fail{se.code, se.msg};
        }
        if (R.failed()) break;
    }
    return R;
}

// The call one batch at a time (hash-table states, Utf8 columns, diagnostics).
Failure run_one_by_one(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins, int32_t nb,
                       uint32_t flags) {
    Failure R;
    for (int32_t b = 0; b < nb; ++b) {
        dfmi_error e{};
        if (dfmi_aggregate_batch(ctx, st, pred, &ins[b], flags, &e) != DFMI_OK) {
            R.batch = b;
            R.fail = Fail{e.code, e.message};
            break;
        }
    }
    return R;
}

// ... through the device hash table (a hash-table state, or a window state
// whose call spans more than the window): one evaluation launch, the
// segments packed dense, the table's passes once per gb::kConcatMaxBatches batches.
Failure run_hashed(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins, int32_t nb,
                   uint32_t flags, const AggDiag& diag) {
    Failure R;
    if (st->acc.p) flush_groups(ctx, st);
    for (int32_t b0 = 0; b0 < nb; b0 += dfmi::gb::kConcatMaxBatches) {
        const int32_t cnt = std::min<int32_t>(dfmi::gb::kConcatMaxBatches, nb - b0);
        int32_t fb = -1;
        try {
            group_batches_hashed(ctx, st, pred, ins + b0, cnt, flags, diag, &fb);
        } catch (const Fail& f) {
            if (fb < 0) throw;  // (not a batch's error: the call's)
            R.batch = b0 + fb;
            R.fail = f;
            break;
        }
    }
    return R;
}

void mm_reset(dfmi_context* ctx, dfmi_agg_state* st) {
    dfmi_error e{};
    if (dfmi_agg_state_reset(ctx, st->mm_state, &e) != DFMI_OK) throw Fail{e.code, e.message};
}

// A key-window state: one window for batches [0, nb).
Failure run_window(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins, int32_t nb,
                   uint32_t flags, const AggDiag& diag) {
    int64_t rows = 0;
    for (int32_t b = 0; b < nb; ++b) rows += ins[b].num_rows;
    if (rows > 0) {
        uint64_t wbase = 0;
        int wwidth = 2;  // Boolean keys: always [false, true]
        if (st->key.type != DFMI_TYPE_BOOLEAN) {
            // integer keys: 16 values from the call's smallest selected key --
            // MIN / MAX of the key over every batch's selected rows, one launch
            wwidth = st->gslots - 1;
            const Failure P = run_batched(ctx, st->mm_state, pred, ins, nb, flags, diag);
            if (P.failed()) {
                // the predicate or the key failed at batch f: evaluated before
                // any aggregate of that batch, but an earlier batch may still
                // hold an argument error, which the reference raises first
                mm_reset(ctx, st);
                const Failure E = run_window(ctx, st, pred, ins, P.batch, flags, diag);
                return E.failed() ? E : P;
            }
            dfmi_error e2{};
            dfmi_agg_value mm[2];
            if (dfmi_agg_state_finish(ctx, st->mm_state, mm, &e2) != DFMI_OK) throw Fail{e2.code, e2.message};
            mm_reset(ctx, st);
            const bool cover =
                st->win_width == wwidth && (mm[0].count == 0 || ((mm[0].bits - st->win_base) < (uint64_t)wwidth &&
                                                                 (mm[1].bits - st->win_base) < (uint64_t)wwidth));
            if (cover) {
                wbase = st->win_base;
            } else {
                wbase = mm[0].count ? mm[0].bits : 0;
                // wider than the device window: the whole call through the hash table
                if (mm[0].count && mm[1].bits - mm[0].bits >= (uint64_t)wwidth)
                    return run_hashed(ctx, st, pred, ins, nb, flags, diag);
            }
        }
        if (st->win_width != wwidth || st->win_base != wbase) {
            flush_groups(ctx, st);
            st->win_base = wbase;
            st->win_width = wwidth;
        }
    }
    const Failure R = run_batched(ctx, st, pred, ins, nb, flags, diag);
    if (rows > 0) st->dirty = true;
    return R;
}

bool reads_utf8(const dfmi_program* p) {
    if (!p) return false;
    if (p->type == DFMI_TYPE_UTF8) return true;
    for (const IrNode& nd : p->ir)
        if (nd.kind == IR_COL && nd.type == DFMI_TYPE_UTF8) return true;
    return false;
}

// The device form's body (the arguments checked, the schema shared).
void aggregate_batches(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins, int32_t nb,
                       uint32_t flags, int32_t* failed) {
    check_not_failed(st);
    const AggDiag diag = agg_diag();
    bool one_by_one = nb == 1 || reads_utf8(pred) || (st->grouped && diag.group_host);
    for (const dfmi_program& k : st->keys) one_by_one = one_by_one || reads_utf8(&k);
    for (const dfmi_aggregate* a : st->aggs) one_by_one = one_by_one || reads_utf8(&a->arg);
    Failure R;
    if (one_by_one) {
        R = run_one_by_one(ctx, st, pred, ins, nb, flags);  // (fails the state itself)
    } else {
        if (st->grouped) unflatten(st);  // a finish's flat groups back in the map before more rows merge
        Unsliced us_;  // sliced arrays (arrow offsets): offset-0 views / shifted bitmaps (slice.cpp)
        if (any_offset(ins, nb)) {
            HIP_TRY(hipSetDevice(ctx->device));
            ins = unslice(ins, nb, us_, true, ctx->stream);
        }
        if (!st->grouped) R = run_batched(ctx, st, pred, ins, nb, flags, diag);
        else if (st->acc.p) R = run_window(ctx, st, pred, ins, nb, flags, diag);
        else R = run_hashed(ctx, st, pred, ins, nb, flags, diag);
        if (R.failed()) {  // the query has failed (the state holds partial sums of the call)
            st->failed = true;
            set_err(&st->failure, R.fail.code, R.fail.msg);
        }
    }
    if (R.failed()) {
        *failed = R.batch;
        throw R.fail;
    }
}

// Bytes of a needed host column's buffers in the staging block (a bitmap without nulls is not staged).
ColBytes staged_bytes(const dfmi_column& c, int64_t n) {
    ColBytes cb = n > 0 ? col_bytes(c, n) : ColBytes{};
    if (c.null_count <= 0) cb.validity = 0;
    return cb;
}

}  // namespace

void dfmi::agg::count_query_launch() { g_query_launches.fetch_add(1, std::memory_order_relaxed); }

extern "C" int32_t dfmi_aggregate_batches(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred,
                                          const dfmi_batch* ins, int32_t nb, uint32_t flags, int32_t* failed,
                                          dfmi_error* err) {
    int32_t dummy_failed;
    if (!failed) failed = &dummy_failed;
    *failed = -1;
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || nb < 0 || (nb > 0 && !ins)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (nb == 0) return DFMI_OK;
        check_shared_schema(ins, nb, false);
        aggregate_batches(ctx, st, pred, ins, nb, flags, failed);
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_aggregate_host_batches(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred,
                                               const dfmi_batch* ins, int32_t nb, uint32_t flags, int32_t* failed,
                                               dfmi_error* err) {
    int32_t dummy_failed;
    if (!failed) failed = &dummy_failed;
    *failed = -1;
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !st || nb < 0 || (nb > 0 && !ins)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (nb == 0) return DFMI_OK;
        check_shared_schema(ins, nb, false);
        check_not_failed(st);
        Unsliced us_;
        if (any_offset(ins, nb)) ins = unslice(ins, nb, us_, false, nullptr);
        const int ncols = ins[0].num_columns;
        std::vector<char> need(ncols, 0);
        mark_columns(pred, need);
        for (const dfmi_program& k : st->keys) mark_columns(&k, need);
        for (const dfmi_aggregate* a : st->aggs) mark_columns(&a->arg, need);
        HIP_TRY(hipSetDevice(ctx->device));
        std::vector<dfmi_column> dcols;
        std::vector<dfmi_batch> dins;
        for (int32_t b0 = 0; b0 < nb;) {
            // ---- the sub-call [b0, b1): whole batches within the staging budget (one over-size batch alone)
            size_t bytes = 0;
            int32_t b1 = b0;
            for (; b1 < nb; ++b1) {
                size_t bb = 0;
                for (int i = 0; i < ncols; ++i) {
                    const dfmi_column& c = ins[b1].columns[i];
                    if (!need[i]) continue;
                    if (ins[b1].num_rows > 0 && (!c.values || (c.type == DFMI_TYPE_UTF8 && !c.offsets)))
                        throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values pointer is NULL"};
                    const ColBytes cb = staged_bytes(c, ins[b1].num_rows);
                    bb += align64(cb.values) + align64(cb.validity) + align64(cb.offsets);
                }
                if (b1 > b0 && bytes + bb > kStageBudget) break;
                bytes += bb;
            }
            // ---- packed into pinned memory, moved with one copy
            st->stage_host.resize(bytes + 64);
            uint8_t* const hbase = st->stage_host.data();
            uint8_t* const dbase = (uint8_t*)st->stage_dev.reserve(bytes + 64);
            dcols.assign((size_t)(b1 - b0) * std::max(ncols, 1), dfmi_column{});
            dins.assign((size_t)(b1 - b0), dfmi_batch{});
            size_t pos = 0;
            auto put = [&](const void* src, size_t n) -> const uint8_t* {
                if (!n) return dbase;  // (non-NULL: nothing of it is read)
                memcpy(hbase + pos, src, n);
                const uint8_t* d = dbase + pos;
                pos += align64(n);
                return d;
            };
            for (int32_t b = b0; b < b1; ++b) {
                dfmi_column* dc = &dcols[(size_t)(b - b0) * std::max(ncols, 1)];
                const int64_t n = ins[b].num_rows;
                for (int i = 0; i < ncols; ++i) {
                    const dfmi_column& c = ins[b].columns[i];
                    dfmi_column& d = dc[i];
                    d = c;
                    d.offset = 0;
                    d.validity = nullptr;
                    d.null_count = 0;
                    d.values = dbase;  // (a column nothing reads: its type and length only)
                    d.offsets = c.type == DFMI_TYPE_UTF8 ? (const int32_t*)dbase : nullptr;
                    if (!need[i]) continue;
                    const ColBytes cb = staged_bytes(c, n);
                    d.values = put(c.values, cb.values);
                    if (cb.validity) {
                        d.validity = put(c.validity, cb.validity);
                        d.null_count = c.null_count;
                    }
                    if (c.type == DFMI_TYPE_UTF8) d.offsets = (const int32_t*)put(c.offsets, cb.offsets);
                }
                dins[(size_t)(b - b0)] = dfmi_batch{ncols, 0, n, dc};
            }
            if (pos) HIP_TRY(hipMemcpyAsync(dbase, hbase, pos, hipMemcpyHostToDevice, ctx->stream));
            try {
                aggregate_batches(ctx, st, pred, dins.data(), b1 - b0, flags, failed);
            } catch (const Fail&) {
                if (*failed >= 0) *failed += b0;
                throw;
            }
            b0 = b1;
        }
        return DFMI_OK;
    });
}

// Internal test hook (not part of the C ABI, not declared in include/): the
// aggregate query-kernel launches of this process -- dfmi_aggregate_batch's one
// per batch, a coalesced call's one per pass.
extern "C" long dfmi_internal_agg_query_launches() { return g_query_launches.load(); }
