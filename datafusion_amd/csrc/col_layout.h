// What a column's buffers weigh and which columns a program reads: the host
// arithmetic shared by every path that stages host columns (host_plan.cpp,
// host_batches.cpp, agg_batches.cpp) or walks them (csv_reader.cpp,
// slice.cpp, sort.cpp, jit_*.cpp). Host only: no HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/dfmi.h"
#include "dfmi_program.h"

namespace dfmi {

// Bytes per value of a fixed-width dfmi_type (0: Boolean, Utf8, anything else).
inline int type_width(int t) {
    switch (t) {
        case DFMI_TYPE_INT8: case DFMI_TYPE_UINT8: return 1;
        case DFMI_TYPE_INT16: case DFMI_TYPE_UINT16: return 2;
        case DFMI_TYPE_INT32: case DFMI_TYPE_UINT32: case DFMI_TYPE_FLOAT32: return 4;
        case DFMI_TYPE_INT64: case DFMI_TYPE_UINT64: case DFMI_TYPE_FLOAT64: return 8;
        default: return 0;
    }
}

// A bitmap of n bits in whole 64-bit words.
inline size_t bitmap_bytes(int64_t n) { return (size_t)((n + 63) / 64) * 8; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// Bytes of the first `rows` rows of a host column's buffers (Utf8: `rows` is
// the column's length). `validity` is set whenever the column carries a
// bitmap; whether a bitmap without nulls is staged is the caller's choice.
struct ColBytes {
    size_t values = 0, validity = 0, offsets = 0;
};

inline ColBytes col_bytes(const dfmi_column& c, int64_t rows) {
    ColBytes cb;
    if (c.type == DFMI_TYPE_UTF8) {
        cb.offsets = (size_t)(rows + 1) * 4;
        cb.values = c.offsets ? (size_t)std::max<int32_t>(0, c.offsets[rows]) : 0;
    } else if (c.type == DFMI_TYPE_BOOLEAN) {
        cb.values = (size_t)((rows + 7) / 8);
    } else {
        cb.values = (size_t)rows * (size_t)type_width(c.type);
    }
    if (c.validity) cb.validity = (size_t)((rows + 7) / 8);
    return cb;
}

// need[i] = 1 for every input column i the program reads (NULL: none).
inline void mark_columns(const dfmi_program* p, std::vector<char>& need) {
    if (!p) return;
    for (const IrNode& nd : p->ir)
        if (nd.kind == IR_COL && nd.col >= 0 && nd.col < (int)need.size()) need[nd.col] = 1;
}

// nb >= 1 batches share batch 0's column count and types, and no batch is
// ragged; `host_pointers`: their host buffers are there too. Throws Fail.
void check_shared_schema(const dfmi_batch* ins, int32_t nb, bool host_pointers);

}  // namespace dfmi
