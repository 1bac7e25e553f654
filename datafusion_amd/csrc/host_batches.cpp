// Many small HOST batches in one call (csv_sql.rs:49-62 pulls 1024-row
// batches from csv::Reader, in host memory): every batch's buffers are packed
// into one pinned staging region (host threads), moved with ONE H2D copy,
// run as ONE coalesced launch (dfmi_filter_project_batches), and the outputs
// come back with ONE D2H copy -- into one pinned block the result owns
// (dfmi_filter_project_host_batches: num_batches x n columns, batch-major, as
// views into it), or into the caller's own block
// (dfmi_filter_project_host_batches_into).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "batch_stage.h"
#include "col_layout.h"
#include "host_arena.h"
#include "host_plan.h"
#include "slice.h"

using namespace dfmi;
using namespace dfmi::host;
using dfmi::xi::guarded;

namespace {

constexpr size_t kZeroCopyBytes = 8 << 20;  // inputs + batch table read in place up to this size (DFMI_HOST_ZC;
                                             // 256 x 1024-row batches: 1.28 -> 1.00 us per batch, profiles/r04/zc_ab2.log)

// Where a host-batches call's headers and outputs land (pinned host memory,
// with the device-visible addresses the kernel writes through when the call
// is zero-copy). `contiguous`: outputs right after the headers (one D2H).
struct HBTarget {
    uint8_t *hdr_host = nullptr, *hdr_dev = nullptr;
    uint8_t *out_host = nullptr, *out_dev = nullptr;
    bool contiguous = false;
};

uint8_t* device_address(uint8_t* host) {
    void* d = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&d, host, 0));
    return (uint8_t*)d;
}

// Every batch's buffers into the pinned staging region, by the host threads.
void pack_inputs(Arena& A, const dfmi_batch* ins, int32_t nb, const HBLayout& Lo) {
    uint8_t* const pin_in = A.pin.p;
    const int ncols = Lo.ncols;
    Tasks tasks;
    const int ways = std::max(1, std::min(A.pool->ways(), (int)(Lo.in_bytes >> 20) + 1));
    for (int w = 0; w < ways; ++w)
        tasks.push_back([&, w] {
            for (int32_t b = w; b < nb; b += ways)
                for (int i = 0; i < ncols; ++i) {
                    const dfmi_column& c = ins[b].columns[i];
                    const HBLayout::In& L = Lo.lay[(size_t)b * ncols + i];
                    if (L.nval) memcpy(pin_in + L.val, c.values, L.nval);
                    if (L.noff) memcpy(pin_in + L.off, c.offsets, L.noff);
                    if (L.nvld) memcpy(pin_in + L.vld, c.validity, L.nvld);
                }
        });
    A.pool->run(tasks);
}

// The batches and their outputs as the device sees them: inputs at `dev`,
// outputs at `dout`, both laid out by Lo.
void device_views(const dfmi_batch* ins, int32_t nb, const HBLayout& Lo, uint8_t* dev, uint8_t* dout,
                  std::vector<dfmi_column>& dcols, std::vector<dfmi_batch>& dins, std::vector<dfmi_out_column>& douts) {
    const int ncols = Lo.ncols, nout = Lo.nout;
    dcols.resize((size_t)nb * std::max(1, ncols));
    dins.resize(nb);
    for (int32_t b = 0; b < nb; ++b) {
        for (int i = 0; i < ncols; ++i) {
            const dfmi_column& c = ins[b].columns[i];
            const HBLayout::In& L = Lo.lay[(size_t)b * ncols + i];
            dfmi_column& d = dcols[(size_t)b * ncols + i];
            d = c;
            d.values = dev + L.val;
            d.offsets = c.type == DFMI_TYPE_UTF8 ? (const int32_t*)(dev + L.off) : nullptr;
            d.validity = L.nvld ? dev + L.vld : nullptr;
            if (!L.nvld) d.null_count = 0;
        }
        dins[b] = dfmi_batch{ncols, 0, ins[b].num_rows, dcols.data() + (size_t)b * ncols};
    }
    douts.assign((size_t)nb * nout, dfmi_out_column{});
    for (size_t k = 0; k < douts.size(); ++k) {
        const HBLayout::Out& L = Lo.olay[k];
        dfmi_out_column& d = douts[k];
        memset(&d, 0, sizeof d);
        d.values = dout + L.val;
        d.validity = dout + L.vld;
        if (Lo.otype[k % nout] == DFMI_TYPE_UTF8) {
            d.offsets = (int32_t*)(dout + L.off);
            d.data = dout + L.dat;
            d.data_capacity = (int64_t)L.ndat;
        }
    }
}

// The common body: packing, the staged coalesced launch. `target` is asked
// once (H, OB, zero-copy) for the output placement. Returns the launch's
// status; *failed = the first failing batch.
int32_t host_batches_run(dfmi_context* ctx, const dfmi_program* pred, const dfmi_program* const* projs, int32_t np,
                         const dfmi_batch* ins, int32_t nb, uint32_t flags, const HBLayout& Lo,
                         const std::function<HBTarget(size_t H, size_t OB, bool zc)>& target,
                         std::vector<dfmi_out_column>& douts, int32_t* failed, dfmi_error* err, CallProf& prof) {
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Arena& A = arena_of(ctx);
    const size_t OB = Lo.OB, H = Lo.H, IB = Lo.IB, MB = Lo.MB;
    // ---- regions. Device (Arena::hb): this call's half [headers |
    // outputs], the other half's headers zeroed by this call's kernel, and
    // [inputs | batch table]; pinned staging: [inputs | table] (ONE H2D, or
    // none: small calls read it in place); the target: headers + outputs
    // (ONE D2H, or none: a small call's kernel writes them in place).
    A.pin.resize(IB + MB, kGrowExact);
    A.reserve_hb(H, OB, IB + MB, st);
    uint8_t* const pin_in = A.pin.p;
    prof.mark(0);
    pack_inputs(A, ins, nb, Lo);
    // zero-copy inputs (small calls): the kernel reads the inputs and the
    // batch table straight from the pinned staging region over PCIe -- no
    // copy in at all on the call's critical path
    static const int zc_env = [] {
        const char* e = getenv("DFMI_HOST_ZC");
        return e ? atoi(e) : -1;
    }();
    const bool zc = zc_env > 0 || (zc_env < 0 && Lo.in_bytes + MB <= kZeroCopyBytes);
    prof.mark(1);
    const int half = A.hb_half, other = 1 - half;
    const HBTarget T = target(H, OB, zc);
    uint8_t* const dhdr = A.hb_half_base(half) + A.hb_hcap - H;  // the kernel's header atomics
    uint8_t* const dout = zc ? T.out_dev : A.hb_half_base(half) + A.hb_hcap;
    uint8_t* const dev = zc ? A.pin.dev : A.hb_inputs();
    std::vector<dfmi_column> dcols;
    std::vector<dfmi_batch> dins;
    device_views(ins, nb, Lo, dev, dout, dcols, dins, douts);
    // ---- (one H2D), the coalesced launch, (one D2H), one synchronisation
    size_t meta_used = 0;
    hipError_t copy_err = hipSuccess;
    bool cleared = false, hdr_written = false;
    BatchStage stage;
    stage.locate = [&](size_t meta_bytes, size_t hdr_bytes, uint8_t** host_meta, uint8_t** dev_meta,
                       uint8_t** dev_hdr, const uint8_t** host_hdr) {
        if (meta_bytes > MB || hdr_bytes > H) return false;
        meta_used = meta_bytes;
        *host_meta = pin_in + IB;
        *dev_meta = dev + IB;
        *dev_hdr = dhdr;
        *host_hdr = T.hdr_host;
        return true;
    };
    stage.copy_in = [&](hipStream_t s) {
        hipError_t e = hipSuccess;
        if (A.hb_dirty[half])  // headers the other half's last kernel did not zero (an earlier failed call)
            e = hipMemsetAsync(A.hb_half_base(half) + A.hb_hcap - A.hb_dirty[half], 0, A.hb_dirty[half], s);
        if (e == hipSuccess && !zc)
            e = hipMemcpyAsync(dev, pin_in, meta_used ? IB + meta_used : Lo.in_bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) copy_err = e;
        else A.hb_dirty[half] = 0;
    };
    stage.copy_out = [&](hipStream_t s) {
        if (zc && hdr_written) return;  // outputs and headers are in place
        hipError_t e;
        if (T.contiguous && !zc) {  // [headers | outputs] in one copy
            e = hipMemcpyAsync(T.hdr_host, dhdr, H + OB, hipMemcpyDeviceToHost, s);
        } else {
            e = hipMemcpyAsync(T.hdr_host, dhdr, H, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && !zc) e = hipMemcpyAsync(T.out_host, dout, OB, hipMemcpyDeviceToHost, s);
        }
        if (e != hipSuccess) copy_err = e;
    };
    if (zc) {
        stage.hdr_out = (uint64_t*)T.hdr_dev;
        stage.hdr_written = &hdr_written;
    }
    stage.clear_bhdr = (uint64_t*)(A.hb_half_base(other) + A.hb_hcap - A.hb_dirty[other]);
    stage.clear_bhdr_words = (int64_t)(A.hb_dirty[other] / 8);
    stage.cleared = &cleared;
    prof.mark(2);
    const int32_t rc = filter_project_batches_staged(ctx, pred, projs, np, dins.data(), nb, douts.data(), flags, failed,
                                                     err, &stage);
    if (rc != DFMI_OK) (void)hipStreamSynchronize(st);  // (a call that failed after copy_in: drain it)
    prof.mark(3);
    if (cleared) {  // this kernel zeroed the other half's headers; this half's are dirty now
        A.hb_dirty[other] = 0;
        A.hb_dirty[half] = std::max(A.hb_dirty[half], H);
        A.hb_half = other;
    }
    HIP_TRY(copy_err);
    return rc;
}

// Output k of a finished call as a column of the result: a view into the
// result's block, or (an Arc clone of an input column) the caller's own
// column, copied.
void result_column(dfmi_host_result* R, const HBLayout& Lo, const dfmi_batch* ins, size_t k,
                   const dfmi_out_column& d) {
    const int b = (int)(k / Lo.nout), o = (int)(k % Lo.nout);
    dfmi_host_result::Col& c = R->cols[k];
    const HBLayout::Out& L = Lo.olay[k];
    if (d.passthrough_column >= 0) {
        const dfmi_column& src = ins[b].columns[d.passthrough_column];
        const HBLayout::In& I = Lo.lay[(size_t)b * Lo.ncols + d.passthrough_column];
        c.length = src.length;
        c.null_count = I.nvld ? src.null_count : 0;
        c.values = R->pool->get(std::max<size_t>(I.nval, 1));
        if (I.nval) memcpy(c.values.p, src.values, I.nval);
        c.v_values = c.values.p;
        if (src.type == DFMI_TYPE_UTF8) {
            c.offsets = R->pool->get(I.noff);
            memcpy(c.offsets.p, src.offsets, I.noff);
            c.v_offsets = (const int32_t*)c.offsets.p;
            c.data_length = (int64_t)I.nval;
        }
        if (I.nvld) {
            c.validity.assign(src.validity, src.validity + I.nvld);
            c.has_validity = true;
            c.v_validity = c.validity.data();
        }
        return;
    }
    c.length = d.length;
    c.null_count = d.null_count;
    c.data_length = d.data_length;
    uint8_t* const ob = R->arena.p + Lo.H;  // the outputs, after the headers
    c.v_values = ob + (Lo.otype[o] == DFMI_TYPE_UTF8 ? L.dat : L.val);
    c.v_offsets = Lo.otype[o] == DFMI_TYPE_UTF8 ? (const int32_t*)(ob + L.off) : nullptr;
    c.v_validity = ob + L.vld;
}

// The device-visible address of the caller's block if it is pinned (the
// kernel's, or the D2H's, target itself), else NULL.
uint8_t* pinned_block_address(uint8_t* blk, size_t bytes, const CallProf& prof) {
    if (is_pinned(blk, 1) && is_pinned(blk, bytes)) return device_address(blk);
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, blk) == hipSuccess && pa.type == hipMemoryTypeHost &&
        hipPointerGetAttributes(&pa, blk + bytes - 1) == hipSuccess && pa.type == hipMemoryTypeHost)
        return device_address(blk);
    (void)hipGetLastError();
    if (prof.on) {  // diagnostics: a pageable caller block costs a copy of the outputs
        static std::atomic<int> said{0};
        if (said++ < 4) {
            hipPointerAttribute_t a{};
            const hipError_t pe = hipPointerGetAttributes(&a, blk);
            (void)hipGetLastError();
            fprintf(stderr, "dfmi host_batches_into: caller block %p not pinned (attr rc %d type %d), %zu bytes\n",
                    (void*)blk, (int)pe, (int)a.type, bytes);
        }
    }
    return nullptr;
}

// Spread over the host threads, batch-sized pieces.
void run_spread(Arena& A, const Tasks& tasks) {
    if (tasks.empty()) return;
    Tasks parts((size_t)std::min<size_t>(A.pool->ways(), tasks.size()));
    for (size_t w = 0; w < parts.size(); ++w)
        parts[w] = [&, w] {
            for (size_t i = w; i < tasks.size(); i += parts.size()) tasks[i]();
        };
    A.pool->run(parts);
}

}  // namespace

extern "C" int32_t dfmi_filter_project_host_batches(dfmi_context* ctx, const dfmi_program* pred,
                                                    const dfmi_program* const* projs, int32_t np,
                                                    const dfmi_batch* ins, int32_t nb, uint32_t flags,
                                                    dfmi_host_result** out, int32_t* failed, dfmi_error* err) {
    // phases: checks + layout, packing into pinned memory, structs, the staged call, result views
    static thread_local CallProf prof("host_batches");
    prof.start();
    int32_t dummy_failed;
    if (!failed) failed = &dummy_failed;
    *failed = -1;
    dfmi_host_result* R = nullptr;
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !out || nb < 0 || (nb > 0 && !ins) || (np > 0 && !projs))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        *out = nullptr;
        ctx->last_err_key = ~0ull;
        if (!pred && np == 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "neither a predicate nor projections"};
        Unsliced us_;  // sliced arrays (slice.cpp)
        if (nb > 0 && any_offset(ins, nb)) ins = unslice(ins, nb, us_, false, nullptr);
        Arena& A = arena_of(ctx);
        R = new dfmi_host_result();
        R->pool = A.results;
        if (nb == 0) {
            *out = R;
            return DFMI_OK;
        }
        HBLayout Lo;
        hb_layout(pred, projs, np, ins, nb, Lo);
        std::vector<dfmi_out_column> douts;
        dfmi_error e2{};
        // the result's pinned block [headers | outputs]; a small call's kernel
        // writes its outputs there directly (and, one tile per batch, the
        // finished headers too: Launch::hdr_out) -- no copy back at all
        auto target = [&](size_t H, size_t OB, bool zc) {
            R->arena = R->pool->get(H + OB);
            HBTarget T;
            T.hdr_host = R->arena.p;
            T.out_host = R->arena.p + H;
            T.contiguous = true;
            if (zc) {
                T.hdr_dev = device_address(R->arena.p);
                T.out_dev = T.hdr_dev + H;
            }
            return T;
        };
        const int32_t rc = host_batches_run(ctx, pred, projs, np, ins, nb, flags, Lo, target, douts, failed, &e2, prof);
        const int32_t nok = rc == DFMI_OK ? nb : std::max(0, *failed);
        R->cols.resize((size_t)nb * Lo.nout);
        for (size_t k = 0; k < R->cols.size(); ++k) {
            R->cols[k].type = Lo.otype[k % Lo.nout];
            // (a failed call: batches from the failing one are empty)
            if ((int32_t)(k / Lo.nout) < nok) result_column(R, Lo, ins, k, douts[k]);
        }
        *out = R;
        R = nullptr;
        if (rc != DFMI_OK) {
            if (err) *err = e2;
            return rc;
        }
        prof.mark(4);
        prof.done();
        return DFMI_OK;
    }, [&] {
        delete R;
    });
}

extern "C" int32_t dfmi_host_batches_output_bytes(const dfmi_program* pred, const dfmi_program* const* projs,
                                                  int32_t np, const dfmi_batch* ins, int32_t nb, uint32_t flags,
                                                  size_t* bytes, dfmi_error* err) {
    (void)flags;
    return guarded(err, [&]() -> int32_t {
        if (!bytes || nb < 0 || (nb > 0 && !ins) || (np > 0 && !projs))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        *bytes = 0;
        if (!pred && np == 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "neither a predicate nor projections"};
        if (nb == 0) return DFMI_OK;
        Unsliced us_;
        if (any_offset(ins, nb)) ins = unslice(ins, nb, us_, false, nullptr);
        HBLayout Lo;
        hb_layout(pred, projs, np, ins, nb, Lo);
        *bytes = Lo.OB;
        return DFMI_OK;
    });
}

extern "C" int32_t dfmi_filter_project_host_batches_into(dfmi_context* ctx, const dfmi_program* pred,
                                                         const dfmi_program* const* projs, int32_t np,
                                                         const dfmi_batch* ins, int32_t nb, uint32_t flags,
                                                         void* out_block, size_t out_capacity,
                                                         dfmi_out_column* outputs, int32_t* failed, dfmi_error* err) {
    static thread_local CallProf prof("host_batches_into");
    prof.start();
    int32_t dummy_failed;
    if (!failed) failed = &dummy_failed;
    *failed = -1;
    Arena* Ap = nullptr;
    PinnedPool::Blk stage_blk;
    return guarded(err, [&]() -> int32_t {
        if (!ctx || nb < 0 || (nb > 0 && (!ins || !outputs || !out_block)) || (np > 0 && !projs))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        ctx->last_err_key = ~0ull;
        if (!pred && np == 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "neither a predicate nor projections"};
        if (nb == 0) return DFMI_OK;
        if ((uintptr_t)out_block & 63) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "out_block must be 64-byte aligned"};
        Unsliced us_;
        const dfmi_batch* const caller_ins = ins;
        if (any_offset(ins, nb)) ins = unslice(ins, nb, us_, false, nullptr);
        HBLayout Lo;
        hb_layout(pred, projs, np, ins, nb, Lo);
        const int nout = Lo.nout;
        if (out_capacity < Lo.OB)
            throw Fail{DFMI_ERR_CAPACITY, "out_block holds " + std::to_string(out_capacity) + " bytes, the outputs need " +
                                              std::to_string(Lo.OB) + " (dfmi_host_batches_output_bytes)"};
        Arena& A = arena_of(ctx);
        Ap = &A;
        uint8_t* const blk = (uint8_t*)out_block;
        uint8_t* const blk_dev = pinned_block_address(blk, Lo.OB, prof);
        std::vector<dfmi_out_column> douts;
        dfmi_error e2{};
        auto target = [&](size_t H, size_t OB, bool zc) {
            HBTarget T;
            A.hdr_pin.resize(H, Grow{(size_t)64 << 10, 0});
            T.hdr_host = A.hdr_pin.p;
            T.hdr_dev = A.hdr_pin.dev;
            if (blk_dev) {
                T.out_host = blk;
                T.out_dev = blk_dev;
            } else {  // pageable: the library's pinned staging, copied below
                stage_blk = A.results->get(OB);
                T.out_host = stage_blk.p;
                if (zc) T.out_dev = device_address(stage_blk.p);
            }
            return T;
        };
        const int32_t rc = host_batches_run(ctx, pred, projs, np, ins, nb, flags, Lo, target, douts, failed, &e2, prof);
        const int32_t nok = rc == DFMI_OK ? nb : std::max(0, *failed);
        // ---- the outputs as views into the caller's block; a pageable block
        // gets the selected bytes (only those) from the staging block
        Tasks tasks;
        const uint8_t* const src = stage_blk.p;
        for (int32_t b = 0; b < nb; ++b)
            for (int o = 0; o < nout; ++o) {
                const size_t k = (size_t)b * nout + o;
                const HBLayout::Out& L = Lo.olay[k];
                dfmi_out_column& u = outputs[k];
                const dfmi_out_column d = douts[k];
                memset(&u, 0, sizeof u);
                u.type = Lo.otype[o];
                u.passthrough_column = -1;
                if (b >= nok) continue;  // a failed call: batches from the failing one are empty
                if (d.passthrough_column >= 0) {  // the caller's own input column (expression.rs:272-276)
                    const dfmi_column& c = caller_ins[b].columns[d.passthrough_column];
                    u.passthrough_column = d.passthrough_column;
                    u.length = c.length;
                    u.null_count = c.validity ? c.null_count : 0;
                    continue;
                }
                u.length = d.length;
                u.null_count = d.null_count;
                u.data_length = d.data_length;
                u.validity = blk + L.vld;
                const int t = Lo.otype[o];
                size_t nv = 0;
                if (t == DFMI_TYPE_UTF8) {
                    u.offsets = (int32_t*)(blk + L.off);
                    u.data = blk + L.dat;
                    u.data_capacity = (int64_t)L.ndat;
                } else {
                    u.values = blk + L.val;
                    nv = t == DFMI_TYPE_BOOLEAN ? (size_t)(d.length + 7) / 8 : (size_t)d.length * type_width(t);
                }
                if (!src) continue;
                const size_t nb_ = (size_t)(d.length + 7) / 8;
                tasks.emplace_back([=] {
                    if (nv) memcpy(blk + L.val, src + L.val, nv);
                    if (d.null_count > 0) memcpy(blk + L.vld, src + L.vld, nb_);
                    if (t == DFMI_TYPE_UTF8) {
                        memcpy(blk + L.off, src + L.off, (size_t)(d.length + 1) * 4);
                        if (d.data_length) memcpy(blk + L.dat, src + L.dat, (size_t)d.data_length);
                    }
                });
            }
        run_spread(A, tasks);
        if (stage_blk.p) A.results->put(stage_blk);
        if (rc != DFMI_OK) {
            if (err) *err = e2;
            return rc;
        }
        prof.mark(4);
        prof.done();
        return DFMI_OK;
    }, [&] {
        if (Ap && stage_blk.p) Ap->results->put(stage_blk);
    });
}
