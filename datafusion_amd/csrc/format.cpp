// dfmi_format_utf8_batches: CAST to Utf8 over device columns
// (DFMI_FLAG_EXT_CAST with DFMI_FLAG_EXT_CAST_UTF8; kernels in format.hip,
// protocol in format.h, the formatting in format_core.h). The fused pass
// evaluates a cast's child into an ordinary fixed-width output column; this
// call turns such columns -- all batches of a coalesced pull at once -- into
// arrow Utf8 arrays: measure, scan, write, one launch of each per call.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "agg_state.h"
#include "format.h"
#include "format_core.h"
#include "slice.h"

namespace dfmi {
namespace fmtk {
namespace {

// The per-row scratch -- `lens` and `sums`, 8 bytes a padded row together, and the scan's `tmp` -- only grows and
// stays with the context until dfmi_context_destroy, as the sort scratch does: the many calls of a pull loop
// allocate nothing, and a 1e8-row call leaves about 0.8 GB of HBM with the context (include/dfmi.h says so).
struct Scratch {
    HostBuf<uint8_t> htable;  // the column table, pinned (one H2D copy per call)
    DevBuf table, totals;     // per column
    DevBuf lens, sums, tmp;   // per row
    HostBuf<unsigned long long> htotals;
    unsigned long long paths[4] = {0, 0, 0, 0};  // the last call's float rows per fmt::Path (DFMI_DIAG=1)
};

Scratch& scratch(dfmi_context* ctx) {
    if (!ctx->format_scratch) ctx->format_scratch = new Scratch();
    return *(Scratch*)ctx->format_scratch;
}

// DFMI_DIAG=1 DFMI_FORMAT_GRID=n: at most n workgroups per launch (read per call).
unsigned grid_cap() {
    if (!getenv("DFMI_DIAG")) return kMaxGrid;
    const char* e = getenv("DFMI_FORMAT_GRID");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? (unsigned)std::min<int>(v, (int)kMaxGrid) : kMaxGrid;
}

void bad(const char* m) { throw Fail{DFMI_ERR_INVALID_ARGUMENT, m}; }

}  // namespace

int32_t format_utf8_batches(dfmi_context* ctx, const dfmi_column* cols_in, const int64_t* num_rows, int32_t ncols,
                            dfmi_out_column* outs, int64_t* data_lengths, uint32_t flags) {
    if (!(flags & DFMI_FLAG_EXT_CAST) || !(flags & DFMI_FLAG_EXT_CAST_UTF8))
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED,
                   "dfmi_format_utf8_batches needs DFMI_FLAG_EXT_CAST and DFMI_FLAG_EXT_CAST_UTF8"};
    if (!ctx || ncols < 0) bad("dfmi_format_utf8_batches: NULL argument");
    if (ncols == 0) return DFMI_OK;
    if (!cols_in || !num_rows || !outs || !data_lengths) bad("dfmi_format_utf8_batches: NULL argument");
    int64_t total = 0;
    for (int i = 0; i < ncols; ++i) {
        const dfmi_column& c = cols_in[i];
        if (c.type == DFMI_TYPE_UTF8) bad("dfmi_format_utf8_batches: a Utf8 input (CAST of a Utf8 column is the column itself)");
        if (c.type < DFMI_TYPE_BOOLEAN || c.type > DFMI_TYPE_FLOAT64) bad("dfmi_format_utf8_batches: column type");
        if (num_rows[i] < 0 || c.length != num_rows[i] || c.offset < 0) bad("dfmi_format_utf8_batches: column length");
        if (num_rows[i] > 0 && !c.values) bad("dfmi_format_utf8_batches: NULL column buffer");
        if (num_rows[i] > 0 && !outs[i].offsets) bad("dfmi_format_utf8_batches: NULL output offsets");
        if (num_rows[i] > 0 && c.validity && c.null_count > 0 && !outs[i].validity)
            bad("dfmi_format_utf8_batches: NULL output validity");
        total += num_rows[i];
        if (total >= (int64_t(1) << 31))
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: 2^31 or more rows to format"};
    }

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Scratch& S = scratch(ctx);

    // sliced inputs: each column as a one-column batch through slice.cpp
    std::vector<dfmi_batch> wrap((size_t)ncols);
    for (int i = 0; i < ncols; ++i) {
        wrap[i].num_columns = 1;
        wrap[i].reserved = 0;
        wrap[i].num_rows = num_rows[i];
        wrap[i].columns = const_cast<dfmi_column*>(cols_in + i);
    }
    Unsliced U;
    const dfmi_batch* bs = wrap.data();
    if (any_offset(bs, ncols)) bs = unslice(bs, ncols, U, true, st);

    // ---- the column table
    S.htable.resize((size_t)ncols * sizeof(Col));
    Col* hc = (Col*)S.htable.data();
    unsigned tiles = 0;
    for (int i = 0; i < ncols; ++i) {
        const dfmi_column& c = bs[i].columns[0];
        const bool nulls = num_rows[i] > 0 && c.validity && c.null_count > 0;
        Col& k = hc[i];
        k.values = c.values;
        k.validity = nulls ? c.validity : nullptr;
        k.offsets = outs[i].offsets;
        k.data = outs[i].data;
        k.out_validity = nulls ? (unsigned long long*)outs[i].validity : nullptr;
        k.n = (unsigned)num_rows[i];
        k.tile0 = tiles;
        k.type = c.type;
        k.pad = 0;
        tiles += (k.n + kTileRows - 1) / kTileRows;  // (total < 2^31 rows: no overflow)
    }
    const size_t slots = (size_t)tiles * kTileRows + 1;

    // ---- scratch, sized before anything is enqueued on it (a growing buffer drops its contents)
    S.table.reserve((size_t)ncols * sizeof(Col));
    S.lens.reserve(slots * sizeof(unsigned));
    S.sums.reserve(slots * sizeof(unsigned));
    S.totals.reserve(((size_t)2 * ncols + 4) * sizeof(unsigned long long));
    S.htotals.resize((size_t)2 * ncols + 4);
    Args A{};
    A.cols = S.table.as<Col>();
    A.ncols = ncols;
    A.tiles = tiles;
    A.lens = S.lens.as<unsigned>();
    A.sums = S.sums.as<unsigned>();
    A.totals = S.totals.as<unsigned long long>();
    A.paths = getenv("DFMI_DIAG") ? A.totals + 2 * ncols : nullptr;
    size_t tmp_bytes = 0;
    HIP_TRY(scan_lengths(nullptr, &tmp_bytes, A, st));
    S.tmp.reserve(tmp_bytes);

    HIP_TRY(hipMemcpyAsync(S.table.p, hc, (size_t)ncols * sizeof(Col), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(A.totals, 0, ((size_t)2 * ncols + 4) * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(A.lens + (slots - 1), 0, sizeof(unsigned), st));
    const unsigned grid = std::max(1u, std::min(tiles, grid_cap()));
    HIP_TRY(launch_measure(A, grid, st));
    HIP_TRY(hipMemcpyAsync(S.htotals.data(), A.totals, ((size_t)2 * ncols + 4) * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 4; ++k) S.paths[k] = A.paths ? S.htotals[2 * ncols + k] : 0;

    // ---- the bytes each column needs: reported whatever follows
    bool too_long = false, too_small = false;
    for (int i = 0; i < ncols; ++i) {
        const unsigned long long need = S.htotals[2 * i];
        data_lengths[i] = (int64_t)need;
        too_long |= need >= (1ull << 31);
        too_small |= outs[i].data && (int64_t)need > outs[i].data_capacity;
    }
    if (too_long)
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: CAST to Utf8 output of 2^31 or more bytes"};
    if (too_small) throw Fail{DFMI_ERR_CAPACITY, "dfmi_format_utf8_batches: data_capacity too small"};

    HIP_TRY(scan_lengths(S.tmp.p, &tmp_bytes, A, st));
    HIP_TRY(launch_write(A, grid, st));
    for (int i = 0; i < ncols; ++i)
        if (num_rows[i] == 0 && outs[i].offsets) HIP_TRY(hipMemsetAsync(outs[i].offsets, 0, sizeof(int32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < ncols; ++i) {
        dfmi_out_column& o = outs[i];
        o.type = DFMI_TYPE_UTF8;
        o.passthrough_column = -1;
        o.length = num_rows[i];
        o.null_count = hc[i].out_validity ? (int64_t)S.htotals[2 * i + 1] : 0;
        o.data_length = (int64_t)S.htotals[2 * i];
    }
    return DFMI_OK;
}

}  // namespace fmtk

void format_scratch_release(dfmi_context* c) {
    delete (fmtk::Scratch*)c->format_scratch;
    c->format_scratch = nullptr;
}

}  // namespace dfmi

// Diagnostics (DFMI_DIAG=1): the float rows of the last dfmi_format_utf8_batches on ctx by the path that gave
// their digits -- out[1] integer, out[2] short decimal, out[3] the exact big-integer path (out[0] unused).
extern "C" int32_t dfmi_internal_format_paths(const dfmi_context* ctx, uint64_t out[4]) {
    if (!ctx || !ctx->format_scratch || !out) return DFMI_ERR_INVALID_ARGUMENT;
    const dfmi::fmtk::Scratch& S = *(const dfmi::fmtk::Scratch*)ctx->format_scratch;
    for (int k = 0; k < 4; ++k) out[k] = S.paths[k];
    return DFMI_OK;
}

extern "C" int32_t dfmi_format_utf8_batches(dfmi_context* ctx, const dfmi_column* columns, const int64_t* num_rows,
                                            int32_t num_columns, dfmi_out_column* outputs, int64_t* data_lengths,
                                            uint32_t flags, dfmi_error* err) {
    return dfmi::xi::guarded(err, [&]() -> int32_t {
        return dfmi::fmtk::format_utf8_batches(ctx, columns, num_rows, num_columns, outputs, data_lengths, flags);
    });
}
