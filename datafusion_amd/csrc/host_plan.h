// Where everything goes in the host paths: pure functions from batch
// descriptions to offsets and sizes (no device, no allocation beyond their
// own vectors). host_chunks.cpp and host_batches.cpp reserve the regions these
// describe and fill them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/dfmi.h"
#include "dfmi_program.h"

namespace dfmi {
namespace host {

// "p .. p + n can be DMA'd from where it is" (host_mem.h is_pinned).
using PinnedFn = bool (*)(const void* p, size_t n);

// ---------------------------------------------------------------- the chunk pipeline
struct Chunk {
    int64_t r0 = 0, rows = 0;
};

// Rows per chunk: ~48 MiB of input per chunk (a multiple of 512 rows, so
// chunk validity bitmaps start on a 64-bit word); one chunk for a batch up to
// 1.5 chunks. DFMI_HOST_CHUNK_ROWS overrides (tests / diagnostics).
int64_t chunk_rows_for(int64_t n, double in_bytes_per_row);
// [0, n) in chunks of `crows` rows (one empty chunk for n == 0).
std::vector<Chunk> chunks_of(int64_t n, int64_t crows);

// What a dfmi_filter_project_host call computes and reads: the output types
// (RuntimeExpr::get_type, or the input columns), the input column an output
// copies or gathers (-1: none), the outputs that are Arc clones of an input
// column, the input columns the device needs and their bytes per row.
struct Shape {
    int ncols = 0, nout = 0;
    std::vector<int> otype, osrc;
    std::vector<char> passthrough, need;
    double in_bpr = 0;
};
// Checks the projections and the batch's columns on the way (throws Fail).
Shape call_shape(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch& in);

// One device/staging buffer of a chunk: `off` in the slot's input region,
// copied from host `src`.
struct Buf {
    size_t off = 0, bytes = 0;
    const uint8_t* src = nullptr;
    bool direct = false;  // src is pinned: DMA from it, no staging copy
};
// Input buffers of a chunk: staged ones first (one contiguous range, one
// DMA), then the ones DMA'd from pinned caller memory.
struct InPlan {
    std::vector<Buf> bufs;  // per column: values, validity, offsets (bytes == 0: absent)
    size_t staged_bytes = 0, total = 0;
};
InPlan plan_chunk_in(const dfmi_batch& in, const std::vector<char>& need, const Chunk& ch, PinnedFn pinned);

// Output region of a slot (worst case for rows_cap rows); bitmap outputs
// (Boolean values, validity) get a staging index.
struct OutPlan {
    size_t values = 0, validity = 0, offsets = 0, data = 0;
    size_t values_cap = 0, data_cap = 0;
    int bm_values = -1, bm_valid = -1;
};
struct OutRegion {
    std::vector<OutPlan> col;
    size_t bytes = 0;  // >= 256
    int n_bm = 0;
};
OutRegion plan_chunk_out(const Shape& S, const std::vector<InPlan>& inplans, int64_t rows_cap);

// ---------------------------------------------------------------- host batches
// Input and worst-case output layout of one host-batches call.
struct HBLayout {
    struct In {
        size_t val = 0, off = 0, vld = 0, nval = 0, noff = 0, nvld = 0;
    };
    struct Out {
        size_t val = 0, vld = 0, off = 0, dat = 0, ndat = 0;
    };
    int ncols = 0, nout = 0;
    std::vector<int> otype;
    std::vector<In> lay;    // [batch][column]
    std::vector<Out> olay;  // [batch][output], offsets in the output region
    size_t in_bytes = 0, out_bytes = 0;
    size_t OB = 0, H = 0, IB = 0, MB = 0;  // outputs, headers, inputs, batch table (aligned)
};
void hb_layout(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch* ins,
               int32_t nb, HBLayout& Lo);

}  // namespace host
}  // namespace dfmi
