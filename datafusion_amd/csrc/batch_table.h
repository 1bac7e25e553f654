// The batch table of a coalesced launch (exec_batches.cpp: filter + project,
// agg_batches.cpp: aggregate): many batches in ONE launch of the batched form
// of a query kernel. The plan is built once from a "shape" batch; a block
// finds its batch through Args::tile_batch and takes its rows, columns and
// header from its row of Args::batch_ptrs (row layout: jit.h batch_slot_*).
// Tiles never straddle batches, and every batch has its own header.
#pragma once
#include <cstring>
#include <vector>

#include "exec_internal.h"

namespace dfmi {
namespace xi {

// Per-batch header (device, zero when a launch starts), in 8-byte words.
constexpr size_t kBatchHdr = 256;      // bytes
constexpr int kBatchHdrTotals = 0;     // [0..8): selected rows, then the bytes of each Utf8 output
constexpr int kBatchHdrNulls = 8;      // [8..24): null count per output
constexpr int kBatchHdrErr = 24;       // the error word (launch_args.h decode_err_word)
inline const uint64_t* batch_hdr(const uint8_t* hdrs, int32_t b) {
    return (const uint64_t*)(hdrs + (size_t)b * kBatchHdr);
}

inline bool has_nulls(const dfmi_column& c) { return c.validity && c.null_count > 0; }

// The shape batch of a call's (unsliced) batches: the shared column types, a
// column nullable where any batch has nulls in it, the longest batch's rows.
// Its pointers are only non-NULL: a plan reads types and nullability.
struct ShapeBatch {
    std::vector<dfmi_column> shape;
    std::vector<char> nullable;
    int64_t maxn = 0;
    dfmi_batch view{};
    ShapeBatch(const dfmi_batch* ins, int32_t nb);
};

// Which tiles of the launch are whose: batch b's are [first[b], first[b] + tiles[b]).
struct TileLayout {
    std::vector<int64_t> first, tiles;
    int64_t T = 0, max_tiles = 0;
    TileLayout(const dfmi_batch* ins, int32_t nb, int64_t tile_rows);
};

// ctx->ones, the all-valid bitmap of maxn rows (returned), filled where a batch
// has no nulls in a column that other batches have them in.
const void* ensure_ones(dfmi_context* ctx, const ShapeBatch& S, const dfmi_batch* ins, int32_t nb, hipStream_t st);

// The table [nb][words] with the tile map [T] behind it, written on the host
// and copied to the device as one block, and the per-batch headers: in the
// context's buffers (in_context) or where the caller's staging has them.
struct BatchTable {
    const jit::Launch& X;
    const ShapeBatch& S;
    const TileLayout& L;
    const int words;  // per row: nout output slots behind the input slots
    const size_t table_bytes, meta_bytes, hdr_bytes;
    uint8_t *host_meta = nullptr, *dev_meta = nullptr, *dev_hdr = nullptr;
    const uint8_t* host_hdr = nullptr;
    const void* ones = nullptr;  // ensure_ones

    BatchTable(const jit::Launch& x, const ShapeBatch& s, const TileLayout& l, int32_t nb, int nout)
        : X(x), S(s), L(l), words(jit::batch_words(x, nout)), table_bytes((size_t)nb * words * 8),
          meta_bytes(table_bytes + (size_t)l.T * 4), hdr_bytes((size_t)nb * kBatchHdr) {}
    void in_context(dfmi_context* ctx);
    uint64_t valid_of(const dfmi_column& c, int col) const {
        if (!S.nullable[col]) return 0;
        return (uint64_t)(has_nulls(c) ? (const void*)c.validity : ones);
    }
    // Batch b's row: its header, input slots and tiles; the row, for the
    // caller's output slots. Inline: once per batch of a 1024-row stream.
    uint64_t* write_row(int32_t b, const dfmi_batch& in) const {
        uint64_t* row = (uint64_t*)host_meta + (size_t)b * words;
        int32_t* tile_batch = (int32_t*)(host_meta + table_bytes);
        memset(row, 0, (size_t)words * 8);
        uint8_t* const hdr = dev_hdr + (size_t)b * kBatchHdr;
        row[0] = (uint64_t)in.num_rows;
        row[1] = (uint64_t)L.tiles[b] | ((uint64_t)L.first[b] << 32);
        row[2] = (uint64_t)(hdr + kBatchHdrTotals * 8);
        row[3] = (uint64_t)(hdr + kBatchHdrErr * 8);
        for (size_t s = 0; s < X.num_cols.size(); ++s) {
            const dfmi_column& c = in.columns[X.num_cols[s]];
            const int w = dfmi::type_width(c.type);
            if (in.num_rows > 0 && !c.values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values pointer is NULL"};
            if (w && ((uintptr_t)c.values & (w - 1)))
                throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values must be aligned to their width"};
            const int sl = jit::batch_slot_col((int)s);
            row[sl] = (uint64_t)c.values;
            row[sl + 1] = valid_of(c, X.num_cols[s]);
        }
        for (size_t u = 0; u < X.utf8_cols.size(); ++u) {
            const dfmi_column& c = in.columns[X.utf8_cols[u]];
            if (in.num_rows > 0 && (!c.values || !c.offsets))
                throw Fail{DFMI_ERR_INVALID_ARGUMENT, "Utf8 column buffers are NULL"};
            const int sl = jit::batch_slot_utf8(X, (int)u);
            row[sl] = (uint64_t)c.offsets;
            row[sl + 1] = (uint64_t)c.values;
            row[sl + 2] = valid_of(c, X.utf8_cols[u]);
        }
        for (int64_t t = 0; t < L.tiles[b]; ++t) tile_batch[L.first[b] + t] = b;
        return row;
    }
};

}  // namespace xi
}  // namespace dfmi
