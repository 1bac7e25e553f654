// CAST to Utf8 on the device (DFMI_FLAG_EXT_CAST_UTF8): the shapes shared by
// the driver (format.cpp) and the fixed kernels (format.hip); the formatting
// itself is format_core.h.
//
// One call formats many columns (the batches of a coalesced pull). Every
// column is cut into tiles of kTileRows rows and the tiles of all columns are
// numbered in column order, so one launch of each kernel covers the call: a
// workgroup finds its tile's column by a search over `tile0`, and every row of
// a tile is of one column and one type. Slot g = tile * kTileRows + row in
// tile of the two scratch arrays holds the row's byte length (measure pass)
// and the sum of the lengths before it (scan); a column's offsets are the
// differences to its first slot, so the sums may wrap 32 bits while a column
// itself stays below 2^31 bytes.
#ifndef DFMI_FORMAT_H
#define DFMI_FORMAT_H

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dfmi {
namespace fmtk {

constexpr int kTileRows = 256;      // rows per workgroup step: four waves, one 64-row slice each
constexpr int kStageBytes = 2048;   // the LDS image of one slice's output span; a longer span is stored per lane
constexpr unsigned kMaxGrid = 2048; // workgroups per launch; a larger call loops (DFMI_DIAG=1 DFMI_FORMAT_GRID=n caps it)

struct Col {
    const void* values;            // offset-0 fixed-width values / Boolean bitmap
    const uint8_t* validity;       // nullptr: every value valid
    int32_t* offsets;              // out: [n + 1]
    uint8_t* data;                 // out; nullptr: measure only
    unsigned long long* out_validity;  // out, with validity: ceil(n / 64) words
    unsigned n;
    unsigned tile0;                // the column's first tile
    int type;                      // dfmi_type
    int pad;
};

struct Args {
    const Col* cols;
    int ncols;
    unsigned tiles;
    unsigned* lens;                // [tiles * kTileRows + 1]
    unsigned* sums;                // [tiles * kTileRows + 1] exclusive sums of lens
    unsigned long long* totals;    // [2 * ncols] per column: bytes, nulls
    unsigned long long* paths;     // [4] or nullptr: float rows per fmt::Path (diagnostics)
};

// format.hip launchers (asynchronous on `st`)
hipError_t launch_measure(const Args& a, unsigned grid, hipStream_t st);
// lens -> sums; tmp == nullptr: *tmp_bytes only
hipError_t scan_lengths(void* tmp, size_t* tmp_bytes, const Args& a, hipStream_t st);
hipError_t launch_write(const Args& a, unsigned grid, hipStream_t st);

}  // namespace fmtk
}  // namespace dfmi

#endif
