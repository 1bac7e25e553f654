// dfmi_filter_project: host side of the fused Selection + Projection pass.
//
// Plans the pass (exec_plan.cpp), gets the query kernel from the query
// compiler (jit.h), launches it, and maps device error words back to the
// reference's errors (FilterRelation::next filter.rs:46-72, filter()
// filter.rs:80-111, ProjectRelation::next projection.rs:45-66). The context
// is context.cpp, the coalesced form of this call exec_batches.cpp.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_stage.h"
#include "launch_args.h"
#include "slice.h"

namespace dfmi {
hipError_t launch_pack_bools(const uint8_t* bytes, uint8_t* bits, const unsigned long long* count,
                             long long max_rows, hipStream_t st);
hipError_t launch_utf8_copy_rows(const int32_t* offs, const int32_t* spos, const uint8_t* src, uint8_t* out,
                                 const unsigned long long* totals, int chan, long long cap, long long max_rows,
                                 hipStream_t st);
}  // namespace dfmi

using namespace dfmi;
using namespace dfmi::xi;

namespace {

// One call behind its plan: the kernel's Args, what is enqueued behind the
// kernel, the device's error, the results.
struct Call {
    dfmi_context* ctx;
    const dfmi_program* pred;
    const dfmi_batch* in;
    dfmi_out_column* outs;
    Built& B;
    Args A;
    // filtered outputs written as one byte per row and packed into a bitmap
    // after the kernel: Boolean values, and the validity of projections that
    // can produce nulls (fallible CAST)
    std::vector<int> bool_out, valid_out;
    std::vector<uint8_t*> bool_dst;
    bool two_pass = false;  // gather 3: offsets + source starts, then k_utf8_copy_rows
    uint64_t dev_key = ~0ull;  // the device's error: evaluation-order key ...
    int dev_kind = 0;          // ... and ERRK_ kind (0: none)

    int nout() const { return (int)B.plan.outs.size(); }
    void bind_outputs_and_scratch();
    void print_debug_stats() const;
    void launch_and_wait(hipFunction_t fn, CallProf& prof);
    void raise_first_error() const;
    void write_results(bool launch, uint64_t hint_key) const;
};

// The kernel's Args but for the workspace: inputs, literals, and the outputs
// -- the caller's buffers, or the context's scratch where a pass behind the
// kernel produces the caller's.
void Call::bind_outputs_and_scratch() {
    const jit::Launch& X = B.X;
    const int64_t n = in->num_rows;
    for (int o = 0; o < nout(); ++o) {
        const jit::OutSpec& os = B.plan.outs[o];
        if (!pred || os.kind == jit::OutSpec::SKIP || os.kind == jit::OutSpec::UTF8) continue;
        if (os.out_type == DFMI_TYPE_BOOLEAN) bool_out.push_back(o);
        if (os.nullable) valid_out.push_back(o);
    }
    const size_t row_bytes = (size_t)((n + 63) & ~63ll);
    if (!bool_out.empty() || !valid_out.empty())
        ctx->scratch.reserve((bool_out.size() + valid_out.size()) * row_bytes, kCtxDev);
    two_pass = pred && X.gather == 3 && !X.utf8_outs.empty();
    const size_t src_bytes = ((size_t)n * 4 + 255) & ~(size_t)255;  // one i32 source start per row
    if (two_pass) ctx->utf8_src.reserve(X.utf8_outs.size() * src_bytes, kCtxDev);
    memset(&A, 0, sizeof A);
    A.n_rows = n;
    A.n_tiles = (int)B.n_tiles;
    bind_inputs(A, X, in);
    bool_dst.assign(nout(), nullptr);
    for (int o = 0; o < nout(); ++o) {
        A.out[o] = outs[o].values;
        A.out_valid[o] = pred ? nullptr : outs[o].validity;
        A.out_offs[o] = outs[o].offsets;
        A.out_data[o] = outs[o].data;
        A.out_cap[o] = outs[o].data_capacity;
    }
    if (two_pass)
        for (size_t j = 0; j < X.utf8_outs.size(); ++j)
            A.out_src[X.utf8_outs[j].first] = (int*)(ctx->utf8_src.as<uint8_t>() + j * src_bytes);
    for (size_t i = 0; i < bool_out.size(); ++i) {
        bool_dst[bool_out[i]] = (uint8_t*)outs[bool_out[i]].values;
        A.out[bool_out[i]] = ctx->scratch.as<uint8_t>() + i * row_bytes;
    }
    for (size_t i = 0; i < valid_out.size(); ++i)
        A.out_valid[valid_out[i]] = ctx->scratch.as<uint8_t>() + (bool_out.size() + i) * row_bytes;
    bind_literals(A, X);
}

// The diagnostics of DFMI_DEBUG_MODE bits 5 and 2, from the header just read.
void Call::print_debug_stats() const {
    if (A.mode & 32) {
        uint64_t g5[5];
        memcpy(g5, ctx->host_hdr.p + kHdrStats + 64, sizeof g5);
        fprintf(stderr, "dfmi utf8 gather cycles (summed over waves): staging %llu setup %llu zero %llu place %llu "
                "store %llu\n", (unsigned long long)g5[0], (unsigned long long)g5[1], (unsigned long long)g5[2],
                (unsigned long long)g5[3], (unsigned long long)g5[4]);
    }
    if (A.mode & 4) {
        uint64_t st3[3];
        memcpy(st3, ctx->host_hdr.p + kHdrStats, sizeof st3);
        fprintf(stderr, "dfmi look-back: tiles %lld polls %llu sleeps %llu wait %.3f ms (summed over tiles)\n",
                (long long)B.n_tiles, (unsigned long long)st3[0], (unsigned long long)st3[1], st3[2] * 1e-5);
    }
}

// The launch with what follows the kernel, synchronised; the header is in
// ctx->host_hdr afterwards and its error word decoded. A look-back that made
// no progress for 2 s (ERRK_LOOKBACK_TIMEOUT: e.g. the GPU time-sliced away
// from this queue for that long) is relaunched once over a freshly zeroed
// workspace before it is reported as a device error; the relaunch rewrites
// every output.
void Call::launch_and_wait(hipFunction_t fn, CallProf& prof) {
    jit::Launch& X = B.X;
    hipStream_t st = ctx->stream;
    const int64_t n = in->num_rows;
    const int n_chan = pred ? 1 + (int)X.utf8_outs.size() : 0;
    const size_t status_bytes = (size_t)n_chan * B.n_tiles * 8 * X.spread;
    for (int attempt = 0;; ++attempt) {
        const WsLease ws = ws_acquire(ctx, status_bytes, st);
        bind_workspace(A, ws);
        A.status = (unsigned long long*)ws.status;
        if (attempt == 0) {
            A.mode = 0;
            if (getenv("DFMI_DIAG"))
                if (const char* m = getenv("DFMI_DEBUG_MODE")) A.mode = atoi(m);  // diagnostics only
        }
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev0, st));
        launch_query(fn, (unsigned)B.n_tiles, X.BLOCK, A, st);  // one block per tile
        ws_commit(ctx, ws);
        if (two_pass && !(A.mode & 8))
            for (size_t j = 0; j < X.utf8_outs.size(); ++j) {
                const int o = X.utf8_outs[j].first;
                HIP_TRY(launch_utf8_copy_rows(A.out_offs[o], A.out_src[o], A.bytes[X.utf8_outs[j].second],
                                              A.out_data[o], A.totals, 1 + (int)j, A.out_cap[o], n, st));
            }
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev1, st));
        for (int o = 0; o < nout(); ++o)
            if (bool_dst[o]) HIP_TRY(launch_pack_bools((const uint8_t*)A.out[o], bool_dst[o], A.totals, n, st));
        for (int o : valid_out) HIP_TRY(launch_pack_bools(A.out_valid[o], outs[o].validity, A.totals, n, st));
        prof.mark(2);
        HIP_TRY(hipMemcpyAsync(ctx->host_hdr.p, ws.hdr, kHdrAlloc, hipMemcpyDeviceToHost, st));
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev2, st));
        HIP_TRY(hipStreamSynchronize(st));
        prof.mark(3);
        uint64_t ew;
        memcpy(&ew, ctx->host_hdr.p + kHdrErr, 8);
        decode_err_word(ew, dev_key, dev_kind);
        print_debug_stats();
        if (ctx->timing) read_timing(ctx, true);
        if (dev_kind != ERRK_LOOKBACK_TIMEOUT || attempt > 0) break;
        ctx->ws_valid = false;  // status words in an unknown state: re-zero all
        ++ctx->relaunches;
        A.mode &= ~16;          // (diagnostic forced timeout: once)
        dev_kind = 0;
        dev_key = ~0ull;
        // relaunched with ticket-ordered tiles: every look-back then
        // waits only on running blocks, whatever else holds the CUs
        X.ticket = 1;
        fn = jit::get_kernel(ctx->device, B.plan, X, &ctx->last_compile_ms);
        bind_literals(A, X);  // (that kernel's literal slots)
    }
}

// The error the reference raises first in evaluation order, the device's or
// the plan's static one.
void Call::raise_first_error() const {
    const Err& se = B.se;
    if (dev_kind == ERRK_LOOKBACK_TIMEOUT) throw Fail{DFMI_ERR_DEVICE, "device look-back timed out"};
    if (dev_kind == ERRK_CAPACITY) throw Fail{DFMI_ERR_CAPACITY, "Utf8 output data_capacity too small"};
    if (dev_kind && (!se.set || dev_key < se.key)) {
        ctx->last_err_key = dev_key;
        throw device_fail(dev_kind);
    }
    if (se.set) {
        ctx->last_err_key = se.key;
        throw Fail{se.code, se.msg};
    }
}

// The outputs' lengths and counts from the header's totals (zero without a
// launch); the selectivity hint of the shape's next large batch.
void Call::write_results(bool launch, uint64_t hint_key) const {
    const jit::Launch& X = B.X;
    uint64_t totals[24];
    memset(totals, 0, sizeof totals);
    if (launch) memcpy(totals, ctx->host_hdr.p + kHdrTotals, sizeof totals);
    const int64_t out_rows = pred ? (int64_t)totals[0] : in->num_rows;
    if (hint_key && launch) sel_hint_update(ctx, hint_key, X, in->num_rows, out_rows, totals[1]);
    for (int o = 0; o < nout(); ++o) {
        dfmi_out_column& oc = outs[o];
        if (oc.passthrough_column >= 0) continue;
        oc.length = out_rows;
        oc.null_count = (!pred || B.plan.outs[o].nullable) ? (int64_t)totals[8 + o] : 0;
        if (B.plan.outs[o].kind == jit::OutSpec::UTF8) {
            oc.data_length = 0;
            for (size_t j = 0; j < X.utf8_outs.size(); ++j)
                if (X.utf8_outs[j].first == o) oc.data_length = (int64_t)totals[1 + j];
            if (!launch) {  // offsets = [0] (a launch writes the final offset itself)
                if (oc.offsets) HIP_TRY(hipMemsetAsync(oc.offsets, 0, 4, ctx->stream));
                oc.data_length = 0;
            }
        }
    }
    if (!launch) HIP_TRY(hipStreamSynchronize(ctx->stream));
}

}  // namespace

extern "C" int32_t dfmi_filter_project(dfmi_context* ctx, const dfmi_program* pred,
                                       const dfmi_program* const* projs, int32_t np,
                                       const dfmi_batch* in, dfmi_out_column* outs, uint32_t flags,
                                       dfmi_error* err) {
    if (ctx) ctx->last_err_key = ~0ull;
    // phases: checks + plan, kernel lookup, enqueue, synchronisation, results
    static thread_local CallProf prof("filter_project");
    prof.start();
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !in || (np > 0 && !projs) || !outs || (in->num_columns > 0 && !in->columns))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        if (!pred && np == 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "neither a predicate nor projections"};
        Unsliced us_;  // sliced arrays (arrow offsets): offset-0 views / shifted bitmaps (slice.cpp)
        if (any_offset(in, 1)) {
            HIP_TRY(hipSetDevice(ctx->device));
            in = unslice(in, 1, us_, true, ctx->stream);
        }
        Built B;
        const uint64_t hint_key = sel_hint_lookup(ctx, pred, projs, np, in, flags, B);
        build_plan(pred, projs, np, in, outs, flags, B);
        if (ctx->shared) B.X.ticket = 1;  // shared GPU: ticket-ordered tiles from the start
        prof.mark(0);

        // ---- compile (cached per query shape) and launch
        HIP_TRY(hipSetDevice(ctx->device));
        ctx->timed = false;
        ctx->last_compile_ms = 0;
        const bool launch = in->num_rows > 0 && (pred || B.any_kernel_out);
        Call c{ctx, pred, in, outs, B};
        if (launch) {
            const hipFunction_t fn = query_kernel(ctx, B.plan, B.X, B.se);
            prof.mark(1);
            c.bind_outputs_and_scratch();
            c.launch_and_wait(fn, prof);
        }
        c.raise_first_error();
        c.write_results(launch, hint_key);
        prof.mark(4);
        prof.done();
        return DFMI_OK;
    });
}
