// The once-per-call parts of a coalesced launch's batch table (batch_table.h).
#include "batch_table.h"

#include <algorithm>

namespace dfmi {
namespace xi {

ShapeBatch::ShapeBatch(const dfmi_batch* ins, int32_t nb)
    : shape(ins[0].num_columns), nullable(ins[0].num_columns, 0) {
    static const uint64_t kDummy[2] = {0, 0};
    const int ncols = ins[0].num_columns;
    for (int32_t b = 0; b < nb; ++b) maxn = std::max<int64_t>(maxn, ins[b].num_rows);
    for (int i = 0; i < ncols; ++i) {
        for (int32_t b = 0; b < nb; ++b)
            if (has_nulls(ins[b].columns[i])) nullable[i] = 1;
        dfmi_column& c = shape[i];
        c = ins[0].columns[i];
        c.length = maxn;
        c.offset = 0;
        c.validity = nullable[i] ? (const uint8_t*)kDummy : nullptr;
        c.null_count = nullable[i] ? 1 : 0;
        c.values = kDummy;
        c.offsets = (const int32_t*)kDummy;
    }
    view = dfmi_batch{ncols, 0, maxn, shape.data()};
}

TileLayout::TileLayout(const dfmi_batch* ins, int32_t nb, int64_t tile_rows) : first(nb), tiles(nb) {
    for (int32_t b = 0; b < nb; ++b) {
        tiles[b] = (ins[b].num_rows + tile_rows - 1) / tile_rows;
        first[b] = T;
        T += tiles[b];
        max_tiles = std::max(max_tiles, tiles[b]);
    }
    if (T > 0x7fffffff) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "batch too large"};
}

const void* ensure_ones(dfmi_context* ctx, const ShapeBatch& S, const dfmi_batch* ins, int32_t nb, hipStream_t st) {
    bool need = false;
    for (size_t i = 0; i < S.nullable.size() && !need; ++i)
        if (S.nullable[i])
            for (int32_t b = 0; b < nb; ++b)
                if (!has_nulls(ins[b].columns[i])) need = true;
    const size_t bytes = (size_t)((S.maxn + 63) / 64 * 8 + 64);
    if (need && ctx->ones.cap < bytes) {
        ctx->ones.reserve(bytes, kCtxDev);
        HIP_TRY(hipMemsetAsync(ctx->ones.p, 0xff, ctx->ones.cap, st));
    }
    return ctx->ones.p;
}

void BatchTable::in_context(dfmi_context* ctx) {
    ctx->host_bmeta.resize(meta_bytes, kCtxPinned);
    ctx->host_bhdr.resize(hdr_bytes, kCtxPinned);
    host_meta = ctx->host_bmeta.p;
    dev_meta = (uint8_t*)ctx->bmeta.reserve(meta_bytes, kCtxDev);
    dev_hdr = (uint8_t*)ctx->bhdr.reserve(hdr_bytes, kCtxDev);
    host_hdr = ctx->host_bhdr.p;
}

}  // namespace xi
}  // namespace dfmi
