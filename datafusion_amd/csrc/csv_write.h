// CSV output on the device (DFMI_FLAG_EXT_CSV_WRITE): the shapes shared by the
// driver (csv_write.cpp) and the fixed kernels (csv_write.hip); the field rules
// are csv_field.h, the numbers' bytes format_core.h.
//
// One call encodes many batches of one column-type list (the batches of a
// coalesced pull) into ONE byte stream, row-major: every batch is cut into
// tiles of kTileRows rows and the tiles of all batches are numbered in batch
// order, so one launch of each kernel covers the call: a workgroup finds its
// tile's batch by a search over `tile0`. Slot g = tile * kTileRows + row in
// tile of the two scratch arrays holds the record's byte length, separators
// and newline included (measure pass), and the bytes before it (scan): the
// record's place in the stream. The slots are 32-bit, so a call stays below
// 2^31 bytes; the driver checks that on the 64-bit batch totals before the scan.
#ifndef DFMI_CSV_WRITE_H
#define DFMI_CSV_WRITE_H

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dfmi {
namespace csvk {

constexpr int kTileRows = 256;       // rows per workgroup step: four waves, one 64-row slice each
constexpr int kImageBytes = 4096;    // the LDS image of one slice's output span; a longer span is stored per lane
constexpr int kScanBytes = 16;       // bytes per lane and load of the quote scan
constexpr unsigned kMaxGrid = 2048;  // workgroups per launch; a larger call loops (DFMI_DIAG=1 DFMI_CSV_GRID=n caps it)
constexpr int kMaxColumns = 256;
constexpr unsigned kQuoteFlag = 0x80000000u;  // of a row's quote word: a ',', '\n' or '\r' (the low bits count its '"')

struct Col {                       // one column of one batch (offset 0: slice.cpp)
    const void* values;            // fixed-width values / Boolean bitmap / Utf8 bytes
    const uint8_t* validity;       // nullptr: every value valid
    const int32_t* offsets;        // Utf8: [n + 1]
    unsigned* quote;               // Utf8: the batch's quote words of this column, [n] (quote scan)
    int type;                      // dfmi_type
    int pad;
};

struct Batch {
    unsigned n;                    // rows
    unsigned tile0;                // the batch's first tile
};

struct Args {
    const Batch* batches;
    const Col* cols;               // [nbatches * ncols], batch-major
    int nbatches, ncols;
    unsigned tiles;
    const int* utf8_cols;          // [nutf8] the schema's Utf8 columns
    int nutf8, pad;
    unsigned* lens;                // [tiles * kTileRows + 1]
    unsigned* sums;                // [tiles * kTileRows + 1] exclusive sums of lens
    unsigned long long* totals;    // [nbatches] bytes per batch
    uint8_t* data;                 // the stream (write pass)
};

// csv_write.hip launchers (asynchronous on `st`)
hipError_t launch_quote_scan(const Args& a, unsigned grid, hipStream_t st);
hipError_t launch_measure(const Args& a, unsigned grid, hipStream_t st);
// lens -> sums; tmp == nullptr: *tmp_bytes only
hipError_t scan_lengths(void* tmp, size_t* tmp_bytes, const Args& a, hipStream_t st);
hipError_t launch_write(const Args& a, unsigned grid, hipStream_t st);

}  // namespace csvk
}  // namespace dfmi

#endif
