// Internals shared by the execution entry points (exec.cpp and
// exec_batches.cpp: filter + project, aggregate.cpp and agg_hash.cpp: the
// aggregate extension): the context (context.cpp), the workspace layout,
// error plumbing.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

#include "buffers.h"
#include "col_layout.h"
#include "dfmi_program.h"
#include "jit.h"

namespace dfmi {
struct Arena;  // host_arena.h
void host_arena_release(dfmi_context* c);  // host_chunks.cpp
}  // namespace dfmi

// Workspace header layout (device, zero when a launch starts).
static constexpr size_t kHdrTicket = 0;
static constexpr size_t kHdrErr = 8;
static constexpr size_t kHdrTotals = 16;
static constexpr size_t kHdrStats = 256;  // look-back statistics (DFMI_DEBUG_MODE bit 4)
static constexpr size_t kHdrAlloc = 512;

struct dfmi_context {
    int device = 0;
    hipStream_t stream = nullptr;
    // Look-back workspace, double-buffered: [hdr 0 | hdr 1 | status 0 | status 1].
    // Launch i uses pair (i & 1), whose first `need` status bytes must be
    // zero on entry; its blocks zero what launch i-1 dirtied in the other
    // pair, for launch i+1 (stream order makes launch i-1 complete first) --
    // no memset per call. Bytes [dirty_lo[b], dirty_hi[b]) of status buffer b
    // may be non-zero. A launch clears the other pair only up to a few times
    // its own status size (a 1024-row call after a 1e9-row call must not
    // zero 31 MB from one block); a larger leftover is cleared by memset of
    // just the prefix a later launch needs (ws_acquire).
    dfmi::DevBuf ws;
    size_t status_cap = 0;       // bytes per status buffer
    int parity = 0;              // pair the next launch uses
    size_t dirty_lo[2] = {0, 0}, dirty_hi[2] = {0, 0};
    bool ws_valid = false;       // the invariant above holds (else re-zero everything)
    dfmi::DevBuf scratch;   // Boolean output bytes (filtered)
    dfmi::DevBuf utf8_src;  // two-pass Utf8 gather: source start per selected row
    dfmi::HostBuf<uint8_t> host_hdr;  // pinned copy of the header
    bool timing = true;  // record HIP events around launches (dfmi_context_set_timing)
    // the GPU is shared with other processes (dfmi_context_set_shared, or
    // DFMI_SHARED=1 at creation): look-back kernels take their tiles in
    // ticket order from the first launch instead of after a 2 s timeout
    bool shared = false;
    dfmi::Arena* host_arena = nullptr;  // the host paths' staging arena (host_arena.h; per context: no shared state)
    void* sort_scratch = nullptr;  // sort.cpp's device scratch, kept across dfmi_sort_batches calls
    void* format_scratch = nullptr;  // format.cpp's, kept across dfmi_format_utf8_batches calls
    void* csv_scratch = nullptr;  // csv_write.cpp's, kept across dfmi_csv_encode_batches calls
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    double last_total_ms = 0, last_main_ms = 0, last_compile_ms = 0;
    bool timed = false;
    // evaluation-order key (ordinal << 44 | row << 4) of the error the last
    // dfmi_filter_project raised; ~0 for none / an error outside that order
    uint64_t last_err_key = ~0ull;
    long relaunches = 0;      // look-back timeouts relaunched (dfmi_internal_relaunches)
    std::string last_kernel;  // name of the last launched query kernel (dfmi_last_kernel_name)
    // coalesced batches (dfmi_filter_project_batches): per-call batch table
    // and per-batch headers, device + pinned host mirrors; an all-valid
    // bitmap for batches without validity in a column others have it for
    dfmi::DevBuf bmeta, bhdr, ones;
    dfmi::HostBuf<uint8_t> host_bmeta, host_bhdr;
    // selectivity of each query shape's last large batch (exec_plan.cpp
    // kSubtileMinRows): picks the sub-tile kernel for low selectivity
    std::unordered_map<uint64_t, double> sel_hint;
    // ... and the mean bytes of its first Utf8 output's selected strings
    // (picks the ring-staged gather, which stages whole 256-row steps)
    std::unordered_map<uint64_t, double> utf8_len_hint;
};

namespace dfmi {
namespace xi {

// (set_err and the entry points' error frame: abi_guard.h; HIP_TRY: buffers.h)

inline bool gatherable(int t, uint32_t flags) {
    if (t == DFMI_TYPE_FLOAT64 || t == DFMI_TYPE_UTF8) return true;  // filter.rs:84,94
    // extension: every fixed-width type and Boolean
    if (flags & DFMI_FLAG_EXT_GATHER_ALL) return is_numeric_type(t) || t == DFMI_TYPE_BOOLEAN;
    return false;
}

// A candidate error: the reference raises the one with the smallest ordinal.
struct Err {
    bool set = false;
    uint64_t key = ~0ull;  // ordinal << 44 | row << 4
    int32_t code = 0;
    std::string msg;
    void offer(uint64_t k, int32_t c, const std::string& m) {
        if (!set || k < key) {
            set = true;
            key = k;
            code = c;
            msg = m;
        }
    }
};

// The context's buffers grow to what a call needs, with a floor and no slack.
constexpr Grow kCtxDev{(size_t)1 << 20, 0}, kCtxPinned{(size_t)1 << 16, 0};

// One launch's share of the double-buffered workspace (see dfmi_context):
// its header and status buffer (zero on entry) and what its blocks clear for
// the next launch.
struct WsLease {
    int par = 0;
    size_t status_bytes = 0;
    uint8_t* hdr = nullptr;
    uint8_t* status = nullptr;
    uint8_t* clear_status = nullptr;  // first status word the kernel zeroes ...
    long long clear_words = 0;        // ... and how many
    uint8_t* clear_hdr = nullptr;
};

inline WsLease ws_acquire(dfmi_context* ctx, size_t status_bytes, hipStream_t st) {
    uint8_t* ws = ctx->ws.as<uint8_t>();
    if (!ws || status_bytes > ctx->status_cap) {
        const size_t cap = (std::max(status_bytes, (size_t)1 << 20) + 255) & ~(size_t)255;
        ws = (uint8_t*)ctx->ws.reserve(2 * kHdrAlloc + 2 * cap, kCtxDev);
        ctx->status_cap = cap;
        ctx->ws_valid = false;
    }
    if (!ctx->ws_valid) {  // first use, growth, or an interrupted call
        HIP_TRY(hipMemsetAsync(ws, 0, 2 * kHdrAlloc + 2 * ctx->status_cap, st));
        ctx->dirty_lo[0] = ctx->dirty_lo[1] = ctx->dirty_hi[0] = ctx->dirty_hi[1] = 0;
        ctx->ws_valid = true;
    }
    WsLease l;
    const int p = ctx->parity, q = 1 - p;
    l.par = p;
    l.status_bytes = status_bytes;
    l.hdr = ws + p * kHdrAlloc;
    l.status = ws + 2 * kHdrAlloc + p * ctx->status_cap;
    // the prefix this launch needs must be zero: what is left dirty in this
    // pair is cleared whole, by one memset (so a small launch after a large
    // one pays it once, not on every later use of the pair)
    size_t& lo = ctx->dirty_lo[p];
    size_t& hi = ctx->dirty_hi[p];
    if (hi > lo && lo < status_bytes) {
        HIP_TRY(hipMemsetAsync(l.status + lo, 0, hi - lo, st));
        lo = hi = 0;
    }
    // what this launch's blocks zero in the other pair (bounded by its size);
    // a larger leftover (a full-table launch before a 1024-row one) is
    // cleared here once, by one memset, and later launches are back to
    // clearing in the kernel
    uint8_t* other = ws + 2 * kHdrAlloc + q * ctx->status_cap;
    size_t& qlo = ctx->dirty_lo[q];
    size_t& qhi = ctx->dirty_hi[q];
    if (qhi > qlo && qhi - qlo > std::max<size_t>(4 * status_bytes, (size_t)64 << 10)) {
        HIP_TRY(hipMemsetAsync(other + qlo, 0, qhi - qlo, st));
        qlo = qhi = 0;
    }
    const size_t qd = qhi - qlo;
    if (qd > 0) {
        l.clear_status = other + qlo;
        l.clear_words = (long long)(qd / 8);
    } else {
        l.clear_status = other;
        l.clear_words = 0;
    }
    l.clear_hdr = ws + q * kHdrAlloc;
    ctx->ws_valid = false;  // until the launch is enqueued (ws_commit)
    return l;
}

// The launch using `l` is enqueued: its status prefix is dirty, and the
// other pair's range it zeroes is clean for the next launch.
inline void ws_commit(dfmi_context* ctx, const WsLease& l) {
    const int p = l.par, q = 1 - p;
    if (l.status_bytes) {
        ctx->dirty_hi[p] = std::max(ctx->dirty_hi[p], l.status_bytes);
        ctx->dirty_lo[p] = 0;
    }
    if (l.clear_words) ctx->dirty_lo[q] = ctx->dirty_hi[q] = 0;
    ctx->parity = q;
    ctx->ws_valid = true;
}

// ---------------------------------------------------------------- planning
// What the filter + project plan (exec_plan.cpp) and the aggregate plan
// (aggregate.cpp build_agg_plan) have in common: the schema checks, the
// static errors of a predicate and of a program at an ordinal base (the
// reference's evaluation order: FilterRelation::next filter.rs:46-72, then
// each expression over the filtered batch), the input slot registration and
// the limits both kernels share.

inline void check_schema(const dfmi_program* p, const dfmi_batch* in) {
    if ((int)p->schema_types.size() != in->num_columns)
        throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batch does not match the compiled schema"};
    for (int i = 0; i < in->num_columns; ++i)
        if (p->schema_types[i] != in->columns[i].type)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batch column type does not match the schema"};
}

inline void check_not_ragged(const dfmi_batch* in) {
    for (int i = 0; i < in->num_columns; ++i)
        if (in->columns[i].length != in->num_rows) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "ragged batch"};
}

// The errors every evaluation of `prog` raises, its nodes' ordinals from `base`.
inline void offer_program_errors(const dfmi_program* prog, int base, Err& se) {
    for (const IrNode& nd : prog->ir)
        if (nd.rt_code) se.offer((uint64_t)(base + nd.ordinal) << 44, nd.rt_code, nd.rt_msg);
}

// ... and a Selection's: the predicate's own nodes, then its type (ordinal
// P), then the columns filter() cannot gather (P + 1). The expressions behind
// it start at ordinal P + 2, which is returned (2 without a predicate).
inline int offer_filter_errors(const dfmi_program* pred, const dfmi_batch* in, uint32_t flags, Err& se) {
    if (!pred) return 2;
    const int P = pred->length;
    offer_program_errors(pred, 0, se);
    if (pred->type != DFMI_TYPE_BOOLEAN)
        se.offer((uint64_t)P << 44, DFMI_ERR_EXECUTION, "Filter expression did not evaluate to boolean");
    for (int i = 0; i < in->num_columns; ++i)
        if (!gatherable(in->columns[i].type, flags)) {
            se.offer((uint64_t)(P + 1) << 44, DFMI_ERR_EXECUTION,
                     std::string("filter not supported for ") + type_debug(in->columns[i].type));
            break;
        }
    return P + 2;
}

// `end`: the ordinal behind the plan's last expression (the error key holds 19 bits of it).
inline void check_ordinal_limit(int end) {
    if (end >= (1 << 19)) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: expressions too long"};
}

// Input columns to the launch's slots, each column once, in the order asked
// for: predicate columns first, then the ones only the outputs read.
struct Slots {
    jit::Launch& X;
    void num(int col, std::vector<int>& phase) {
        for (int c : X.num_cols)
            if (c == col) return;
        X.num_cols.push_back(col);
        phase.push_back((int)X.num_cols.size() - 1);
    }
    int utf8(int col) {
        for (size_t i = 0; i < X.utf8_cols.size(); ++i)
            if (X.utf8_cols[i] == col) return (int)i;
        X.utf8_cols.push_back(col);
        return (int)X.utf8_cols.size() - 1;
    }
    void prog(const dfmi_program* p, std::vector<int>& phase) {
        for (const IrNode& nd : p->ir) {
            if (nd.kind != IR_COL) continue;
            if (nd.type == DFMI_TYPE_UTF8) utf8(nd.col);
            else if (dfmi::type_width(nd.type) || nd.type == DFMI_TYPE_BOOLEAN) num(nd.col, phase);
        }
    }
    void check_limit(int max_num, int max_utf8) const {  // (the kernel's Args: kArgCols, kArgUtf8)
        if ((int)X.num_cols.size() > max_num || (int)X.utf8_cols.size() > max_utf8)
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: too many input columns"};
    }
};

// Tiles of `tile_rows` rows that cover n rows (a launch's grid: 31 bits).
inline int64_t tiles_of(int64_t n, int64_t tile_rows) {
    const int64_t t = (n + tile_rows - 1) / tile_rows;
    if (t > 0x7fffffff) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "batch too large"};
    return t;
}

// A device limit (NotImplemented) found while planning is reported only when
// the plan raises none of the reference's own errors first: those come
// earlier in its evaluation order (and stand for what it would report).
template <class F>
inline void static_error_first(const Err& se, F&& plan) {
    try {
        plan();
    } catch (const Fail& f) {
        if (f.code == DFMI_ERR_NOT_IMPLEMENTED && se.set) throw Fail{se.code, se.msg};
        throw;
    }
}

// ------------------------------------------- the filter + project plan
// (exec_plan.cpp), as its launch sites use it: dfmi_filter_project (exec.cpp)
// and the coalesced form (exec_batches.cpp).

// Everything about one call that does not need the device: static errors,
// output metadata, the jit plan and the column slot tables.
struct Built {
    Err se;
    jit::Plan plan;
    jit::Launch X;
    bool any_kernel_out = false;
    int64_t n_tiles = 0;
    bool low_sel = false;  // in: this query shape selected few rows last time (dfmi_context::sel_hint)
    bool high_sel = false;  // in: ... or at least kLowSel of them
    bool ring_ok = false;  // in: ... selected many rows with short Utf8 strings (the ring-staged gather)
    bool long_utf8 = false;  // in: ... selected long Utf8 strings (the long per-lane fallback copy)
};

// Fills B (its hint flags are inputs) and the outputs' metadata; a static
// error wins over a device limit (static_error_first).
void build_plan(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch* in,
                dfmi_out_column* outs, uint32_t flags, Built& B);

// What the query shape's last large batch on this context selected, into B's
// hint flags; the shape's key, 0 when the batch is too small to keep one.
uint64_t sel_hint_lookup(const dfmi_context* ctx, const dfmi_program* pred, const dfmi_program* const* projs,
                         int32_t np, const dfmi_batch* in, uint32_t flags, Built& B);
// ... and what this batch selected (out_rows of n rows, utf8_bytes in its
// first Utf8 output), for the shape's next one.
void sel_hint_update(dfmi_context* ctx, uint64_t key, const jit::Launch& X, int64_t n, int64_t out_rows,
                     uint64_t utf8_bytes);

}  // namespace xi
}  // namespace dfmi
