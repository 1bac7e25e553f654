// dfmi_filter_project over many batches in ONE launch (include/dfmi.h). Each
// batch keeps its own outputs, row counts and errors: tiles never straddle
// batches, a batch's tiles run the single-pass look-back over their own
// status segment, and every batch has its own header (totals, null counts,
// error word). The plan is built once from a "shape" batch -- the shared
// column types, a column nullable when any batch has nulls in it
// (batch_table.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_stage.h"
#include "batch_table.h"
#include "launch_args.h"
#include "slice.h"

using namespace dfmi;
using namespace dfmi::xi;

namespace {

// One call's arguments (the batches unsliced), and whether its table and
// headers are in the caller's staging (one copy each way with its own data)
// and not in the context's buffers.
struct Call {
    dfmi_context* ctx;
    const dfmi_program* pred;
    const dfmi_batch* ins;
    int32_t nb;
    dfmi_out_column* outs;  // [nb][nout]
    int nout;
    const BatchStage* stage;
    bool staged = false;
};

int32_t batches_one_by_one(const Call& c, const dfmi_program* const* projs, int32_t np, uint32_t flags,
                           int32_t* failed, dfmi_error* err) {
    for (int32_t b = 0; b < c.nb; ++b) {
        const int32_t rc =
            dfmi_filter_project(c.ctx, c.pred, projs, np, &c.ins[b], c.outs + (size_t)b * c.nout, flags, err);
        if (rc != DFMI_OK) {
            *failed = b;
            return rc;
        }
    }
    return DFMI_OK;
}

// A plan that fails statically, gathers in two passes, launches nothing, or
// has filtered Boolean / nullable outputs (packed per batch after the kernel)
// runs one batch at a time.
bool runs_one_by_one(const Built& B, const dfmi_program* pred) {
    if (B.se.set || B.X.gather == 3 || !(pred || B.any_kernel_out)) return true;
    if (pred)
        for (const jit::OutSpec& os : B.plan.outs)
            if (os.kind != jit::OutSpec::SKIP && os.kind != jit::OutSpec::UTF8 &&
                (os.out_type == DFMI_TYPE_BOOLEAN || os.nullable))
                return true;
    return false;
}

// The batch table: every batch's row (batch_table.h) with its output slots.
void write_table(const Call& c, const jit::Plan& plan, const BatchTable& table) {
    for (int32_t b = 0; b < c.nb; ++b) {
        check_not_ragged(&c.ins[b]);
        uint64_t* row = table.write_row(b, c.ins[b]);
        for (int o = 0; o < c.nout; ++o) {
            const dfmi_out_column& oc = c.outs[(size_t)b * c.nout + o];
            const jit::OutSpec& os = plan.outs[o];
            const int sl = jit::batch_slot_out(table.X, o);
            if (os.kind == jit::OutSpec::UTF8) {
                if (!oc.offsets || !oc.data) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "Utf8 output buffers are NULL"};
            } else if (os.kind != jit::OutSpec::SKIP) {
                if (!oc.values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "output values pointer is NULL"};
                if (!c.pred && !oc.validity)
                    throw Fail{DFMI_ERR_INVALID_ARGUMENT, "output validity pointer is NULL"};
            }
            row[sl] = (uint64_t)oc.values;
            row[sl + 1] = c.pred ? 0 : (uint64_t)oc.validity;
            row[sl + 2] = (uint64_t)oc.offsets;
            row[sl + 3] = (uint64_t)oc.data;
            row[sl + 4] = (uint64_t)oc.data_capacity;
        }
    }
}

// The launch, synchronised. A look-back that timed out in any batch (the GPU
// time-sliced away from this queue for 2 s) is relaunched once over a
// re-zeroed workspace and headers, as dfmi_filter_project does; the relaunch
// rewrites every batch's outputs.
void launch_batches(const Call& c, const jit::Plan& plan, jit::Launch& X, hipFunction_t fn, const BatchTable& table,
                    CallProf& prof) {
    dfmi_context* ctx = c.ctx;
    const BatchStage* stage = c.stage;
    hipStream_t st = ctx->stream;
    const int64_t T = table.L.T;
    if (stage) stage->copy_in(st);  // (staged: with the table; headers zeroed by the previous call)
    int mode = 0;
    if (getenv("DFMI_DIAG"))
        if (const char* m = getenv("DFMI_DEBUG_MODE")) mode = atoi(m);  // diagnostics only (bit 4: force a timeout)
    for (int attempt = 0;; ++attempt) {
        if (T > 0) {
            if (!c.staged && attempt == 0)
                HIP_TRY(hipMemcpyAsync(table.dev_meta, table.host_meta, table.meta_bytes, hipMemcpyHostToDevice, st));
            if (!c.staged || attempt > 0) HIP_TRY(hipMemsetAsync(table.dev_hdr, 0, table.hdr_bytes, st));
            const int n_chan = c.pred ? 1 + (int)X.utf8_outs.size() : 0;
            const size_t status_bytes = (size_t)n_chan * T * 8 * X.spread;
            Args A;
            memset(&A, 0, sizeof A);
            A.n_rows = table.S.maxn;
            A.n_tiles = (int)T;
            A.mode = mode;
            bind_literals(A, X);
            const WsLease ws = ws_acquire(ctx, status_bytes, st);
            bind_workspace(A, ws);
            A.status = (unsigned long long*)ws.status;
            A.tile_batch = (const int*)(table.dev_meta + table.table_bytes);
            A.batch_ptrs = (void* const*)table.dev_meta;
            if (stage) {
                A.clear_bhdr = (unsigned long long*)stage->clear_bhdr;
                A.clear_bhdr_words = stage->clear_bhdr_words;
                if (X.hdr_out) A.hdr_out = (unsigned long long*)stage->hdr_out;
            }
            if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev0, st));
            launch_query(fn, (unsigned)T, X.BLOCK, A, st);
            ws_commit(ctx, ws);
            if (stage && stage->cleared) *stage->cleared = true;
            if (X.hdr_out && stage->hdr_written) *stage->hdr_written = true;
            if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev1, st));
            if (!c.staged)
                HIP_TRY(hipMemcpyAsync(ctx->host_bhdr.p, ctx->bhdr.p, table.hdr_bytes, hipMemcpyDeviceToHost, st));
        }
        for (int32_t b = 0; b < c.nb; ++b)  // empty batches: Utf8 offsets = [0]
            if (c.ins[b].num_rows == 0)
                for (int o = 0; o < c.nout; ++o)
                    if (plan.outs[o].kind == jit::OutSpec::UTF8 && c.outs[(size_t)b * c.nout + o].offsets)
                        HIP_TRY(hipMemsetAsync(c.outs[(size_t)b * c.nout + o].offsets, 0, 4, st));
        if (stage) stage->copy_out(st);  // (staged: with the headers)
        prof.mark(3);
        HIP_TRY(hipStreamSynchronize(st));
        prof.mark(4);
        bool timed_out = false;
        for (int32_t b = 0; b < c.nb && T > 0; ++b) {
            const uint64_t ew = c.ins[b].num_rows > 0 ? batch_hdr(table.host_hdr, b)[kBatchHdrErr] : 0;
            if (ew && (int)(~ew & 15) == ERRK_LOOKBACK_TIMEOUT) timed_out = true;
        }
        if (!timed_out || attempt > 0) break;
        ctx->ws_valid = false;  // status words in an unknown state: re-zero all
        ++ctx->relaunches;
        mode &= ~16;  // (diagnostic forced timeout: once)
        X.ticket = 1;  // ticket-ordered tiles (see dfmi_filter_project)
        fn = jit::get_kernel(ctx->device, plan, X, &ctx->last_compile_ms);
    }
    if (T > 0 && ctx->timing) read_timing(ctx, false);
}

// Per batch, in order: its results, or the first failing batch's error.
void batch_results(const Call& c, const jit::Plan& plan, const BatchTable& table, int32_t* failed) {
    const jit::Launch& X = table.X;
    for (int32_t b = 0; b < c.nb; ++b) {
        const uint64_t* h = batch_hdr(table.host_hdr, b);
        const bool ran = c.ins[b].num_rows > 0;
        if (const uint64_t ew = ran ? h[kBatchHdrErr] : 0) {
            const uint64_t key = ~ew;
            const int kind = (int)(key & 15);
            *failed = b;
            if (kind == ERRK_LOOKBACK_TIMEOUT) throw Fail{DFMI_ERR_DEVICE, "device look-back timed out"};
            if (kind == ERRK_CAPACITY) throw Fail{DFMI_ERR_CAPACITY, "Utf8 output data_capacity too small"};
            c.ctx->last_err_key = key & ~15ull;
            throw device_fail(kind);
        }
        const int64_t n = c.ins[b].num_rows;
        const int64_t out_rows = c.pred ? (ran ? (int64_t)h[kBatchHdrTotals] : 0) : n;
        for (int o = 0; o < c.nout; ++o) {
            dfmi_out_column& oc = c.outs[(size_t)b * c.nout + o];
            const dfmi_out_column& tmpl = c.outs[o];
            oc.type = tmpl.type;
            oc.passthrough_column = tmpl.passthrough_column;
            oc.data_length = 0;
            if (oc.passthrough_column >= 0) {  // Arc clone of this batch's column
                const dfmi_column& col = c.ins[b].columns[oc.passthrough_column];
                oc.length = n;
                oc.null_count = col.validity ? col.null_count : 0;
                continue;
            }
            oc.length = out_rows;
            oc.null_count = (!c.pred && ran) ? (int64_t)h[kBatchHdrNulls + o] : 0;
            if (plan.outs[o].kind == jit::OutSpec::UTF8 && ran)
                for (size_t j = 0; j < X.utf8_outs.size(); ++j)
                    if (X.utf8_outs[j].first == o) oc.data_length = (int64_t)h[kBatchHdrTotals + 1 + j];
        }
    }
}

}  // namespace

extern "C" int32_t dfmi_filter_project_batches(dfmi_context* ctx, const dfmi_program* pred,
                                               const dfmi_program* const* projs, int32_t np, const dfmi_batch* ins,
                                               int32_t nb, dfmi_out_column* outs, uint32_t flags,
                                               int32_t* failed, dfmi_error* err) {
    return dfmi::filter_project_batches_staged(ctx, pred, projs, np, ins, nb, outs, flags, failed, err, nullptr);
}

int32_t dfmi::filter_project_batches_staged(dfmi_context* ctx, const dfmi_program* pred,
                                            const dfmi_program* const* projs, int32_t np, const dfmi_batch* ins,
                                            int32_t nb, dfmi_out_column* outs, uint32_t flags, int32_t* failed,
                                            dfmi_error* err, const BatchStage* stage) {
    // phases: checks + plan, kernel lookup, batch table, enqueue, synchronisation, results
    static thread_local CallProf prof("batches_staged");
    prof.start();
    int32_t dummy_failed;
    if (!failed) failed = &dummy_failed;
    *failed = -1;
    if (ctx) ctx->last_err_key = ~0ull;
    return guarded(err, [&]() -> int32_t {
        if (!ctx || nb < 0 || (nb > 0 && (!ins || !outs)) || (np > 0 && !projs))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (!pred && np == 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "neither a predicate nor projections"};
        if (nb == 0) return DFMI_OK;
        Unsliced us_;  // sliced arrays (slice.cpp)
        if (any_offset(ins, nb)) {
            HIP_TRY(hipSetDevice(ctx->device));
            ins = unslice(ins, nb, us_, true, ctx->stream);
        }
        const int ncols = ins[0].num_columns;
        for (int32_t b = 0; b < nb; ++b) {
            if (ins[b].num_columns != ncols || (ncols > 0 && !ins[b].columns))
                throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batches do not share a schema"};
            for (int i = 0; i < ncols; ++i)
                if (ins[b].columns[i].type != ins[0].columns[i].type)
                    throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batches do not share a schema"};
        }
        Call c{ctx, pred, ins, nb, outs, np > 0 ? np : ncols, stage};
        const ShapeBatch S(ins, nb);
        Built B;
        build_plan(pred, projs, np, &S.view, outs, flags, B);
        if (ctx->shared) B.X.ticket = 1;  // shared GPU: ticket-ordered tiles from the start
        jit::Launch& X = B.X;
        if (runs_one_by_one(B, pred)) {
            if (stage) {
                HIP_TRY(hipSetDevice(ctx->device));
                stage->copy_in(ctx->stream);
            }
            const int32_t rc = batches_one_by_one(c, projs, np, flags, failed, err);
            if (stage) {
                stage->copy_out(ctx->stream);
                HIP_TRY(hipStreamSynchronize(ctx->stream));
            }
            return rc;
        }

        X.batched = true;
        HIP_TRY(hipSetDevice(ctx->device));
        ctx->timed = false;
        ctx->last_compile_ms = 0;
        const TileLayout L(ins, nb, (int64_t)X.BLOCK * X.K * X.M);
        BatchTable table(X, S, L, nb, c.nout);  // (its layout does not depend on hdr_out)
        c.staged = stage && stage->locate &&
                   stage->locate(table.meta_bytes, table.hdr_bytes, &table.host_meta, &table.dev_meta, &table.dev_hdr,
                                 &table.host_hdr);
        // one tile per batch and a staged caller that takes the headers in
        // place (decided after locate: an unstaged call reads its headers
        // from ctx->bhdr, which a hdr_out kernel would zero before the D2H)
        X.hdr_out = c.staged && stage->hdr_out && L.max_tiles <= 1;
        prof.mark(0);
        const hipFunction_t fn = jit::get_kernel(ctx->device, B.plan, X, &ctx->last_compile_ms);
        ctx->last_kernel = X.kname;
        prof.mark(1);
        if (!c.staged) table.in_context(ctx);
        table.ones = ensure_ones(ctx, S, ins, nb, ctx->stream);
        write_table(c, B.plan, table);
        prof.mark(2);
        launch_batches(c, B.plan, X, fn, table, prof);
        batch_results(c, B.plan, table, failed);
        prof.mark(5);
        prof.done();
        return DFMI_OK;
    });
}
