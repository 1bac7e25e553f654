// Marshalling of one query-kernel launch, shared by the launch sites
// (dfmi_filter_project, filter_project_batches_staged, dfmi_aggregate_batch):
// the kernel's Args bound from the batch, the plan's literal pools and the
// workspace lease; the launch; the error word decoded. All inline: the
// per-call path of a 1024-row batch is counted in microseconds.
#pragma once
#include <cstring>

#include "exec_internal.h"
#include "jit_skeleton.hip"

namespace dfmi {

// The text of ERRK_CAST_DIGITS / ERRK_CAST_DIGITS_F32 (DFMI_FLAG_EXT_CAST_ANY).
inline const char* cast_digits_message(int kind) {
    return kind == ERRK_CAST_DIGITS_F32 ? "device program limit: CAST to Float32 needs more than 19 significant digits"
                                        : "device program limit: CAST to Float64 needs more than 19 significant digits";
}
inline bool is_cast_digits(int kind) { return kind == ERRK_CAST_DIGITS || kind == ERRK_CAST_DIGITS_F32; }

// The reference's error (or the device limit) behind an arithmetic or CAST
// ERRK_ kind of a device error word. A look-back timeout and ERRK_CAPACITY
// are the launch sites' own: they mean different things to each.
inline Fail device_fail(int kind) {
    if (kind == ERRK_DIV_ZERO) return Fail{DFMI_ERR_DIVIDE_BY_ZERO, "DivideByZero"};
    if (kind == ERRK_REM_OVERFLOW) return Fail{DFMI_ERR_PANIC, "attempt to calculate the remainder with overflow"};
    if (is_cast_digits(kind)) return Fail{DFMI_ERR_NOT_IMPLEMENTED, cast_digits_message(kind)};
    return Fail{DFMI_ERR_PANIC, "attempt to divide with overflow"};
}

namespace xi {

// The numeric and Utf8 input columns of X's slots.
inline void bind_inputs(Args& A, const jit::Launch& X, const dfmi_batch* in) {
    for (size_t s = 0; s < X.num_cols.size(); ++s) {
        const dfmi_column& c = in->columns[X.num_cols[s]];
        if (!c.values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values pointer is NULL"};
        const int w = dfmi::type_width(c.type);
        if (w && ((uintptr_t)c.values & (w - 1)))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values must be aligned to their width"};
        A.col[s] = c.values;
        A.valid[s] = (c.validity && c.null_count > 0) ? c.validity : nullptr;
    }
    for (size_t u = 0; u < X.utf8_cols.size(); ++u) {
        const dfmi_column& c = in->columns[X.utf8_cols[u]];
        if (!c.values || !c.offsets) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "Utf8 column buffers are NULL"};
        A.offs[u] = c.offsets;
        A.bytes[u] = (const u8*)c.values;
        A.svalid[u] = (c.validity && c.null_count > 0) ? c.validity : nullptr;
    }
}

// The query kernel of (plan, X), compiled on first use. Where the reference
// fails first (`se`, a static error), its error and not the compiler's.
inline hipFunction_t query_kernel(dfmi_context* ctx, const jit::Plan& plan, jit::Launch& X, const Err& se) {
    try {
        const hipFunction_t fn = jit::get_kernel(ctx->device, plan, X, &ctx->last_compile_ms);
        ctx->last_kernel = X.kname;
        return fn;
    } catch (const Fail&) {
        if (se.set) throw Fail{se.code, se.msg};
        throw;
    }
}

// The literal slots of the kernel X names (they differ between kernels).
inline void bind_literals(Args& A, const jit::Launch& X) {
    const jit::LitPool& L = X.lits;
    memcpy(A.lits, L.bits, sizeof A.lits);
    memcpy(A.str_off, L.str_off, sizeof A.str_off);
    memcpy(A.str_len, L.str_len, sizeof A.str_len);
    memcpy(A.str, L.str, sizeof A.str);
}

// The lease's header words and what the launch clears for the next one
// (A.status is the look-back's alone: its callers set it).
inline void bind_workspace(Args& A, const WsLease& ws) {
    A.ticket = (unsigned*)(ws.hdr + kHdrTicket);
    A.err = (unsigned long long*)(ws.hdr + kHdrErr);
    A.totals = (unsigned long long*)(ws.hdr + kHdrTotals);
    A.stats = (unsigned long long*)(ws.hdr + kHdrStats);
    A.clear_status = (unsigned long long*)ws.clear_status;
    A.clear_words = ws.clear_words;
    A.clear_hdr = (unsigned long long*)ws.clear_hdr;
}

inline void launch_query(hipFunction_t fn, unsigned grid, unsigned block, Args& A, hipStream_t stream) {
    size_t asz = sizeof A;
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, stream, nullptr, cfg));
}

// The launch's device times from the context's events: ev0 .. ev1 the
// kernels, ev0 .. ev2 (where the call recorded it) with the header's copy.
inline void read_timing(dfmi_context* ctx, bool has_ev2) {
    float m1 = 0, m2 = 0;
    (void)hipEventElapsedTime(&m1, ctx->ev0, ctx->ev1);
    if (has_ev2) (void)hipEventElapsedTime(&m2, ctx->ev0, ctx->ev2);
    ctx->last_main_ms = m1;
    ctx->last_total_ms = has_ev2 ? m2 : m1;
    ctx->timed = true;
}

// The header's error word (0: none): its evaluation-order key and ERRK_ kind.
inline void decode_err_word(uint64_t ew, uint64_t& dev_key, int& dev_kind) {
    if (!ew) return;
    dev_key = ~ew;
    dev_kind = (int)(dev_key & 15);
    dev_key &= ~15ull;
}

}  // namespace xi
}  // namespace dfmi
