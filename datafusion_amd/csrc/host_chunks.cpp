// dfmi_filter_project_host: the host-buffer form of one FilterRelation /
// ProjectRelation pull, for callers that hold Arrow batches in host memory
// (the Rust reference's arrow 0.12 buffers, csv::Reader output).
//
// Replaces, for a host batch, FilterRelation::next (filter.rs:46-72) +
// filter() (filter.rs:80-111) + ProjectRelation::next (projection.rs:45-66).
//
// Rows are independent (filter.rs:87-91 preserves row order), so a host
// batch is cut into row chunks that flow through a three-stage pipeline over
// three slots (device input + output regions, pinned staging for both):
//
//   host threads : stage-in chunk j      | copy-out chunk j-2
//   H2D stream   : chunk j               (DMA engine, host -> HBM)
//   ctx stream   : fused kernel chunk j-1 (exec.cpp, waits on the H2D event)
//   D2H stream   : results chunk j-1     (DMA engine, HBM -> host)
//
// so both PCIe directions, the kernel and the host copies overlap. Columns
// whose buffers are pinned (dfmi_host_alloc / dfmi_host_register) skip the
// staging copy and are DMA'd straight from the caller's memory. Chunk results
// are concatenated on the host in row order: Utf8 offsets rebased, bitmaps
// bit-shifted; the first error in the reference's evaluation order is taken
// over all chunks (smallest ordinal, then earliest global row).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "col_layout.h"
#include "host_arena.h"
#include "host_bits.h"
#include "host_plan.h"
#include "slice.h"

using namespace dfmi;
using namespace dfmi::host;
using dfmi::xi::guarded;
using dfmi::xi::set_err;

namespace dfmi {
void host_arena_release(dfmi_context* c) {
    delete c->host_arena;
    c->host_arena = nullptr;
}
}  // namespace dfmi

namespace {

// a host batch up to this size skips the chunk pipeline (one H2D, one
// launch, one D2H, one synchronisation: redirect_small)
constexpr int64_t kSmallRows = 1 << 16;
constexpr size_t kSmallBytes = (size_t)4 << 20;

// DFMI_HOST_PROFILE=1: per-call phase times on stderr (diagnostics only).
struct PhaseClock {
    enum { StageIn = 0, Finish = 2, IssueH2D, Kernel, IssueD2H, Drain, Setup };
    bool on = false;
    double t[8] = {};
    std::chrono::steady_clock::time_point t0, call_t0;
    static double ms_since(std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    }
    void start() {
        if (on) t0 = std::chrono::steady_clock::now();
    }
    void stop(int i) {
        if (on) t[i] += ms_since(t0);
    }
};

// What chunk k's kernel left: its output columns, and where its rows and
// Utf8 bytes start in the result.
struct Done {
    std::vector<dfmi_out_column> oc;
    int64_t row_base = 0;
    std::vector<int64_t> byte_base;
};

// The state of one call; one member function per step of the pipeline.
struct ChunkedCall {
    dfmi_context* ctx;
    const dfmi_program* pred;
    const dfmi_program* const* projs;
    int32_t np;
    const dfmi_batch* in;
    uint32_t flags;

    Arena* A = nullptr;
    int ways = 1;
    PhaseClock pc;
    // ---- the plan
    Shape S;
    int64_t n = 0, crows = 0;
    std::vector<Chunk> chunks;
    int nch = 0;
    std::vector<InPlan> inplans;
    OutRegion out;
    size_t in_cap = 0, slot_dev = 0, bm_chunk = 0;
    bool small = false;  // one chunk whose whole output region comes back in one DMA, through pin_small
    PinnedPool::Blk bm_stage;  // per (bitmap output, chunk): the chunk's bitmap, merged bit-shifted in finish
    dfmi_host_result* R = nullptr;
    // ---- progress
    std::vector<Done> done;
    int64_t rows_so_far = 0;
    std::vector<int64_t> bytes_so_far, nulls;
    bool failed = false;
    xi::Err first;  // first error in the reference's evaluation order over all chunks
    Tasks tasks;

    uint8_t* dev_in(int s) const { return A->dev.as<uint8_t>() + (size_t)s * slot_dev; }
    uint8_t* dev_out(int s) const { return dev_in(s) + in_cap; }
    uint8_t* pin_in(int s) const { return A->pin.p + (size_t)s * in_cap; }
    uint8_t* pin_small() const { return A->pin.p + (size_t)kSlots * in_cap; }
    uint8_t* bm_at(int idx, int k) const { return bm_stage.p + ((size_t)idx * nch + k) * bm_chunk; }

    bool redirect_small(dfmi_host_result** out_res, dfmi_error* err, int32_t* rc);
    void plan();
    void stage_in(int k);
    void issue_h2d(int k);
    void run_kernel(int k);
    void issue_d2h(int k);
    void drain();
    void finish_passthrough(int o);
    void finish_small(int o);
    void finish();
    void abandon();
};

// Small batches (csv_sql.rs:49's 1024 rows): no chunk pipeline, copy streams
// or host threads -- the one-batch form of the host-batches path: pack into
// pinned memory, one H2D, the launch and one D2H of the output region on the
// context stream, one sync. true: the call is done, with *rc.
bool ChunkedCall::redirect_small(dfmi_host_result** out_res, dfmi_error* err, int32_t* rc) {
    static const bool chunk_env = getenv("DFMI_HOST_CHUNK_ROWS") != nullptr;
    if (in->num_rows > kSmallRows || chunk_env) return false;
    size_t bytes = 0;
    for (int i = 0; i < in->num_columns; ++i) {
        const dfmi_column& c = in->columns[i];
        bytes += col_bytes(c, c.length).values + (c.validity ? (size_t)(in->num_rows + 7) / 8 : 0) +
                 (c.type == DFMI_TYPE_UTF8 ? (size_t)(in->num_rows + 1) * 4 : 0);
    }
    if (bytes > kSmallBytes) return false;
    int32_t failed_batch = -1;
    *rc = dfmi_filter_project_host_batches(ctx, pred, projs, np, in, 1, flags, out_res, &failed_batch, err);
    if (*rc != DFMI_OK && *out_res) {
        dfmi_host_result_free(*out_res);
        *out_res = nullptr;
    }
    return true;
}

// The chunks, each chunk's input buffers, a slot's output region, the
// device and pinned regions for kSlots slots, and the result's blocks.
void ChunkedCall::plan() {
    HIP_TRY(hipSetDevice(ctx->device));
    A = &arena_of(ctx);
    ways = A->pool->ways();
    pc.on = getenv("DFMI_HOST_PROFILE") != nullptr;
    pc.call_t0 = std::chrono::steady_clock::now();
    n = in->num_rows;
    S = call_shape(pred, projs, np, *in);
    crows = chunk_rows_for(n, S.in_bpr);
    chunks = chunks_of(n, crows);
    nch = (int)chunks.size();
    const int64_t rows_cap = std::max<int64_t>(crows, 1);
    inplans.resize(nch);
    for (int k = 0; k < nch; ++k) {
        inplans[k] = plan_chunk_in(*in, S.need, chunks[k], is_pinned);
        in_cap = std::max(in_cap, inplans[k].total);
    }
    in_cap = std::max<size_t>(in_cap, 256);
    out = plan_chunk_out(S, inplans, rows_cap);
    // a small single chunk returns its whole output region in one DMA
    // (one latency) and is copied into the results on the host
    small = nch == 1 && out.bytes <= ((size_t)1 << 20);
    slot_dev = in_cap + out.bytes;
    A->dev.reserve(slot_dev * kSlots, kGrowExact);
    A->pin.resize(in_cap * kSlots + (small ? out.bytes : 0), kGrowExact);
    bm_chunk = bitmap_bytes(rows_cap);
    if (!small && out.n_bm) bm_stage = A->results->get((size_t)out.n_bm * nch * bm_chunk);

    // ---- results: pinned blocks sized for the worst case (DMA targets)
    R = new dfmi_host_result();
    R->pool = A->results;
    R->cols.resize(S.nout);
    for (int o = 0; o < S.nout; ++o) {
        dfmi_host_result::Col& rc = R->cols[o];
        const int t = rc.type = S.otype[o];
        if (S.passthrough[o]) continue;
        if (t == DFMI_TYPE_UTF8) {
            const size_t total = S.osrc[o] >= 0 ? col_bytes(in->columns[S.osrc[o]], n).values : 0;
            rc.offsets = A->results->get((size_t)(n + 1) * 4);
            ((int32_t*)rc.offsets.p)[0] = 0;
            rc.values = A->results->get(total + 8);
        } else {
            if (t == DFMI_TYPE_BOOLEAN)
                rc.bits.resize((size_t)(n + 7) / 8 + 16);
            else
                rc.values = A->results->get((size_t)n * std::max(type_width(t), 1) + 8);
            rc.validity.resize((size_t)(n + 7) / 8 + 16);
        }
    }
    done.resize(nch);
    bytes_so_far.assign(S.nout, 0);
    nulls.assign(S.nout, 0);
    pc.t[PhaseClock::Setup] = PhaseClock::ms_since(pc.call_t0);
}

// Host threads copy chunk k's pageable buffers into its slot's pinned staging.
void ChunkedCall::stage_in(int k) {
    pc.start();
    tasks.clear();
    uint8_t* pin = pin_in(k % kSlots);
    for (const Buf& b : inplans[k].bufs)
        if (b.bytes && !b.direct) add_copy(tasks, pin + b.off, b.src, b.bytes, ways);
    A->pool->run(tasks);
    pc.stop(PhaseClock::StageIn);
}

void ChunkedCall::issue_h2d(int k) {
    pc.start();
    const int s = k % kSlots;
    const InPlan& P = inplans[k];
    // the slot's inputs were read by the kernel of chunk k - kSlots
    if (A->slot_used[s]) HIP_TRY(hipStreamWaitEvent(A->h2d, A->kdone[s], 0));
    if (P.staged_bytes) HIP_TRY(hipMemcpyAsync(dev_in(s), pin_in(s), P.staged_bytes, hipMemcpyHostToDevice, A->h2d));
    for (const Buf& b : P.bufs)
        if (b.bytes && b.direct) HIP_TRY(hipMemcpyAsync(dev_in(s) + b.off, b.src, b.bytes, hipMemcpyHostToDevice, A->h2d));
    HIP_TRY(hipEventRecord(A->h2d_done[s], A->h2d));
    pc.stop(PhaseClock::IssueH2D);
}

// Chunk k's fused kernel on the context stream (dfmi_filter_project over the
// slot's device columns), once its inputs have landed; an error in the
// reference's evaluation order is kept and the later chunks still run (one
// of them may hold an earlier one).
void ChunkedCall::run_kernel(int k) {
    pc.start();
    const int s = k % kSlots, ncols = S.ncols, nout = S.nout;
    const Chunk& ch = chunks[k];
    const InPlan& P = inplans[k];
    hipStream_t st = ctx->stream;
    std::vector<dfmi_column> dcols(std::max(1, ncols));
    for (int i = 0; i < ncols; ++i) {
        const dfmi_column& c = in->columns[i];
        dfmi_column& d = dcols[i];
        d = c;
        d.length = ch.rows;
        d.values = nullptr;
        d.validity = nullptr;
        d.offsets = nullptr;
        if (!S.need[i]) continue;
        const Buf& v = P.bufs[(size_t)3 * i];
        const Buf& b = P.bufs[(size_t)3 * i + 1];
        const Buf& of = P.bufs[(size_t)3 * i + 2];
        uint8_t* base = dev_in(s);
        if (c.type == DFMI_TYPE_UTF8) {
            d.offsets = (const int32_t*)(base + of.off);
            // offsets stay absolute: the bytes pointer is shifted by the
            // chunk's first offset (the kernel only forms bytes + offset)
            d.values = base + v.off - c.offsets[ch.r0];
        } else {
            d.values = base + v.off;
        }
        if (c.validity) d.validity = base + b.off;
    }
    dfmi_batch db = *in;
    db.num_rows = ch.rows;
    db.columns = dcols.data();
    Done& D = done[k];
    D.oc.assign(std::max(1, nout), dfmi_out_column{});
    uint8_t* ob = dev_out(s);
    for (int o = 0; o < nout; ++o) {
        dfmi_out_column& c = D.oc[o];
        memset(&c, 0, sizeof c);
        if (S.passthrough[o]) continue;
        const OutPlan& p = out.col[o];
        if (S.otype[o] == DFMI_TYPE_UTF8) {
            c.offsets = (int32_t*)(ob + p.offsets);
            c.data = ob + p.data;
            c.data_capacity = (int64_t)p.data_cap;
        } else {
            c.values = ob + p.values;
            c.validity = ob + p.validity;
        }
    }
    HIP_TRY(hipStreamWaitEvent(st, A->h2d_done[s], 0));
    if (A->slot_used[s]) HIP_TRY(hipStreamWaitEvent(st, A->d2h_done[s], 0));  // its output region is free
    dfmi_error e{};
    const int32_t rc = dfmi_filter_project(ctx, pred, projs, np, &db, D.oc.data(), flags, &e);
    if (rc != DFMI_OK) {
        uint64_t key = ctx->last_err_key;
        if (key == ~0ull) throw Fail{rc, e.message};  // outside the evaluation order: fatal now
        if (rc == DFMI_ERR_DIVIDE_BY_ZERO || rc == DFMI_ERR_PANIC) {
            // device error: make the row global (key = ordinal << 44 | row << 4)
            const uint64_t ord = key >> 44, row = ((key >> 4) & ((1ull << 40) - 1)) + (uint64_t)ch.r0;
            key = ord << 44 | row << 4;
        }
        first.offer(key, rc, e.message);
        failed = true;
        pc.stop(PhaseClock::Kernel);
        return;
    }
    // the D2H of these results (and the slot's next H2D) run on other
    // streams: they wait for the kernel on the device, not the host
    HIP_TRY(hipEventRecord(A->kdone[s], st));
    HIP_TRY(hipStreamWaitEvent(A->d2h, A->kdone[s], 0));
    D.row_base = rows_so_far;
    D.byte_base.assign(nout, 0);
    int64_t L = 0;
    for (int o = 0; o < nout; ++o) {
        if (S.passthrough[o]) continue;
        L = D.oc[o].length;
        D.byte_base[o] = bytes_so_far[o];
        bytes_so_far[o] += D.oc[o].data_length;
        nulls[o] += D.oc[o].null_count;
    }
    rows_so_far += L;
    pc.stop(PhaseClock::Kernel);
}

// D2H of chunk k's results straight into the result blocks (bitmaps into
// per-chunk staging, merged bit-shifted at the end).
void ChunkedCall::issue_d2h(int k) {
    if (failed) return;
    pc.start();
    const int s = k % kSlots;
    const Done& D = done[k];
    const uint8_t* dob = dev_out(s);
    auto cp = [&](void* dst, const uint8_t* src, size_t b) {
        if (b) HIP_TRY(hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, A->d2h));
    };
    if (small) {
        cp(pin_small(), dob, out.bytes);
    } else {
        for (int o = 0; o < S.nout; ++o) {
            if (S.passthrough[o]) continue;
            dfmi_host_result::Col& rc = R->cols[o];
            const dfmi_out_column& c = D.oc[o];
            const OutPlan& p = out.col[o];
            const int64_t L = c.length;
            const int t = S.otype[o];
            if (t == DFMI_TYPE_UTF8) {
                cp(rc.offsets.p + (D.row_base + 1) * 4, dob + p.offsets + 4, (size_t)L * 4);
                cp(rc.values.p + D.byte_base[o], dob + p.data, (size_t)c.data_length);
                continue;
            }
            if (t == DFMI_TYPE_BOOLEAN)
                cp(bm_at(p.bm_values, k), dob + p.values, (size_t)(L + 7) / 8);
            else
                cp(rc.values.p + D.row_base * type_width(t), dob + p.values, (size_t)L * type_width(t));
            if (c.null_count > 0) cp(bm_at(p.bm_valid, k), dob + p.validity, (size_t)(L + 7) / 8);
        }
    }
    HIP_TRY(hipEventRecord(A->d2h_done[s], A->d2h));
    A->slot_used[s] = true;
    pc.stop(PhaseClock::IssueD2H);
}

// Every copy has landed; the first error of the chunks, if any, is the call's.
void ChunkedCall::drain() {
    pc.start();
    HIP_TRY(hipStreamSynchronize(A->h2d));
    HIP_TRY(hipStreamSynchronize(A->d2h));
    for (int s = 0; s < kSlots; ++s) A->slot_used[s] = false;
    pc.stop(PhaseClock::Drain);
    if (failed) {
        ctx->last_err_key = first.key;
        throw Fail{first.code, first.msg};
    }
}

// Output o is an Arc clone of an input column (expression.rs:274): copied.
void ChunkedCall::finish_passthrough(int o) {
    dfmi_host_result::Col& rc = R->cols[o];
    const dfmi_column& c = in->columns[S.osrc[o]];
    const ColBytes cb = col_bytes(c, n);
    rc.length = n;
    rc.null_count = c.validity ? c.null_count : 0;
    rc.values = A->results->get(cb.values + 8);
    add_copy(tasks, rc.values.p, c.values, cb.values, ways);
    if (c.validity && c.null_count > 0) {
        rc.validity.resize(cb.validity);
        add_copy(tasks, rc.validity.data(), c.validity, cb.validity, ways);
        rc.has_validity = true;
    } else {
        rc.null_count = 0;
    }
    if (c.type == DFMI_TYPE_UTF8) {
        rc.offsets = A->results->get(cb.offsets);
        add_copy(tasks, rc.offsets.p, c.offsets, cb.offsets, ways);
    }
}

// Output o of the `small` single chunk: out of pin_small into the result.
void ChunkedCall::finish_small(int o) {
    dfmi_host_result::Col& rc = R->cols[o];
    const dfmi_out_column& c = done[0].oc[o];
    const OutPlan& p = out.col[o];
    const uint8_t* src = pin_small();
    const int64_t L = c.length;
    const int t = S.otype[o];
    if (t == DFMI_TYPE_UTF8) {
        add_copy(tasks, rc.offsets.p + 4, src + p.offsets + 4, (size_t)L * 4, ways);
        add_copy(tasks, rc.values.p, src + p.data, (size_t)c.data_length, ways);
        return;
    }
    if (t == DFMI_TYPE_BOOLEAN)
        add_copy(tasks, rc.bits.data(), src + p.values, (size_t)(L + 7) / 8, ways);
    else
        add_copy(tasks, rc.values.p, src + p.values, (size_t)L * type_width(t), ways);
    if (rc.has_validity) add_copy(tasks, rc.validity.data(), src + p.validity, (size_t)(L + 7) / 8, ways);
}

// Utf8 rebase, bitmaps, small-chunk copies, lengths, passthrough copies.
void ChunkedCall::finish() {
    pc.start();
    tasks.clear();
    for (int o = 0; o < S.nout; ++o) {
        if (S.passthrough[o]) {
            finish_passthrough(o);
            continue;
        }
        dfmi_host_result::Col& rc = R->cols[o];
        const int t = S.otype[o];
        rc.length = rows_so_far;
        rc.null_count = nulls[o];
        rc.has_validity = t != DFMI_TYPE_UTF8 && nulls[o] > 0;
        if (t == DFMI_TYPE_UTF8) rc.data_length = bytes_so_far[o];
        if (small) {
            finish_small(o);
            continue;
        }
        if (t == DFMI_TYPE_UTF8) {
            for (int k = 1; k < nch; ++k) {  // chunk offsets start at 0: add the bytes before them
                const Done& D = done[k];
                int32_t* p = (int32_t*)rc.offsets.p + D.row_base + 1;
                add_copy_rebase(tasks, p, p, (size_t)D.oc[o].length, (int32_t)D.byte_base[o], ways);
            }
            continue;
        }
        if (t == DFMI_TYPE_BOOLEAN) {
            tasks.emplace_back([this, o] {
                for (int k = 0; k < nch; ++k)
                    append_bits(R->cols[o].bits.data(), done[k].row_base, bm_at(out.col[o].bm_values, k), done[k].oc[o].length);
            });
        }
        if (rc.has_validity) {
            tasks.emplace_back([this, o] {
                for (int k = 0; k < nch; ++k) {
                    const dfmi_out_column& c = done[k].oc[o];
                    if (c.null_count > 0)
                        append_bits(R->cols[o].validity.data(), done[k].row_base, bm_at(out.col[o].bm_valid, k), c.length);
                    else
                        append_ones(R->cols[o].validity.data(), done[k].row_base, c.length);
                }
            });
        }
    }
    A->pool->run(tasks);
    for (int o = 0; o < S.nout; ++o) {
        dfmi_host_result::Col& rc = R->cols[o];
        if (S.passthrough[o] || S.otype[o] == DFMI_TYPE_UTF8) continue;
        if (S.otype[o] == DFMI_TYPE_BOOLEAN) {
            finish_bitmap(rc.bits.data(), rows_so_far);
            rc.bits.resize((size_t)(rows_so_far + 7) / 8);
        }
        if (rc.has_validity) {
            finish_bitmap(rc.validity.data(), rows_so_far);
            rc.validity.resize((size_t)(rows_so_far + 7) / 8);
        } else {
            rc.validity.clear();
        }
    }
    if (bm_stage.p) A->results->put(bm_stage);
    pc.stop(PhaseClock::Finish);
    if (pc.on)
        fprintf(stderr,
                "dfmi host: %d chunks of %lld rows, setup %.2f ms | stage-in %.2f, issue H2D %.2f, kernel (incl. "
                "wait H2D) %.2f, issue D2H %.2f, drain %.2f, finish %.2f | total %.2f ms\n",
                nch, (long long)crows, pc.t[PhaseClock::Setup], pc.t[PhaseClock::StageIn], pc.t[PhaseClock::IssueH2D],
                pc.t[PhaseClock::Kernel], pc.t[PhaseClock::IssueD2H], pc.t[PhaseClock::Drain], pc.t[PhaseClock::Finish],
                PhaseClock::ms_since(pc.call_t0));
}

// A failed call: the copies in flight drained, the slots and the half-built
// result released.
void ChunkedCall::abandon() {
    if (A) {
        (void)hipStreamSynchronize(A->h2d);
        (void)hipStreamSynchronize(A->d2h);
        for (int s = 0; s < kSlots; ++s) A->slot_used[s] = false;
        if (bm_stage.p) A->results->put(bm_stage);
    }
    delete R;
    R = nullptr;
}

}  // namespace

extern "C" int32_t dfmi_filter_project_host(dfmi_context* ctx, const dfmi_program* pred,
                                            const dfmi_program* const* projs, int32_t np,
                                            const dfmi_batch* in, uint32_t flags,
                                            dfmi_host_result** out, dfmi_error* err) {
    ChunkedCall C{ctx, pred, projs, np, in, flags};
    const auto body = [&]() -> int32_t {
        if (!ctx || !in || !out || (np > 0 && !projs) || (in->num_columns > 0 && !in->columns))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        *out = nullptr;
        ctx->last_err_key = ~0ull;
        Unsliced us_;  // sliced arrays (arrow offsets): offset-0 views / shifted bitmaps (slice.cpp)
        if (any_offset(in, 1)) C.in = unslice(in, 1, us_, false, nullptr);
        if (C.in->num_rows < 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "negative row count"};
        int32_t rc = DFMI_OK;
        if (C.redirect_small(out, err, &rc)) return rc;
        C.plan();
        for (int j = 0; j <= C.nch; ++j) {
            if (j < C.nch) {
                C.stage_in(j);
                C.issue_h2d(j);
            }
            if (j >= 1) {
                C.run_kernel(j - 1);
                C.issue_d2h(j - 1);
            }
        }
        C.drain();
        C.finish();
        *out = C.R;
        return DFMI_OK;
    };
    try {
        return guarded(err, body, [&] { C.abandon(); });
    } catch (const std::bad_alloc&) {
        C.abandon();
        set_err(err, DFMI_ERR_INVALID_ARGUMENT, "host allocation failed");
        return DFMI_ERR_INVALID_ARGUMENT;
    }
}
