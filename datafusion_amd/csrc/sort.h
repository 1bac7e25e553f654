// ORDER BY / LIMIT on the device (DFMI_FLAG_EXT_SORT): the shapes shared by
// the driver (sort.cpp) and the fixed kernels (sort.hip).
//
// A row is a global 32-bit index over the input batches in order; the kernels
// resolve it through `Rows` -- the row prefix of the batches and, per column,
// one `ColPtr` per batch -- so the batches are never concatenated. The sort
// is a permutation of those indices: LSD passes of a stable radix sort over
// (key word, row index), one word at a time from the least significant word
// of the last key to the most significant word of the first, then one gather
// of every column by the permutation.
#ifndef DFMI_SORT_H
#define DFMI_SORT_H

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dfmi {
namespace srt {

constexpr int kMaxKeys = 8;      // ORDER BY expressions
constexpr int kSelectBits = 11;  // radix select: bits per pass
constexpr int kSelectBins = 1 << kSelectBits;
constexpr int kSelectRows = 4096;  // rows per workgroup of the select's histogram / count / compaction kernels
constexpr unsigned kShortString = 16;  // Utf8 gather: longer strings are copied by the whole wave

// One column of one batch (dfmi_column's buffers).
struct ColPtr {
    const void* values;       // fixed-width values / Boolean bitmap / Utf8 bytes
    const uint8_t* validity;  // nullptr: every value valid
    const int32_t* offsets;   // Utf8
    long long offset;         // arrow ArrayData::offset
};

struct Rows {
    const unsigned* prefix;  // [nb + 1] first global row of each batch; prefix[nb] = total rows
    int nb;
    unsigned n;              // total rows
};

// Which word of a key k_sort_word writes.
enum Word : int {
    kWordValue = 0,   // fixed width: sort_value_low, a null row's word 0 (+ the null bit above, `null_above`)
    kWordNull = 1,    // 1 for a null row, else 0
    kWordChunk = 2,   // Utf8: bytes [8 * chunk, 8 * chunk + 8) big-endian, zero-padded; a null row's word 0
    kWordLength = 3,  // Utf8: the byte length; a null row's word 0
    kWordSelect = 4   // the leading word in 64 bits (fixed width: sort_value_low, with nulls a bit above for
                      // <= 32-bit types; Utf8: chunk 0), a null row's word all ones: monotone with the full order
};

struct WordArgs {
    Rows rows;
    const ColPtr* col;     // [nb] the key column
    int type;              // dfmi_type
    int what;              // Word
    int chunk;             // kWordChunk
    int asc;               // 0: the word is complemented
    int has_nulls;         // some batch's column has nulls
    int null_above;        // kWordValue / kWordSelect: the null bit sits at bit sort_value_bits(type)
    const unsigned* perm;  // nullptr: row i (and perm_out[i] = i)
    unsigned* perm_out;    // with perm == nullptr
    unsigned n;            // words to write
    unsigned long long* words;
};

struct SelectState {       // device words of the radix select
    unsigned long long prefix;  // the k-th word's bits found so far
    unsigned long long k;       // rank still to find among the rows that share `prefix` (1-based)
    unsigned long long total;   // k_sort_offsets: candidates
    unsigned long long pad;
};

struct GatherArgs {
    Rows rows;
    const ColPtr* col;     // [nb]
    const unsigned* perm;
    unsigned m;            // output rows
    void* out;
};

struct BitsArgs {
    Rows rows;
    const ColPtr* col;
    const unsigned* perm;
    unsigned m;
    int validity;          // 1: the validity bitmaps (a batch without one: all valid); 0: Boolean values
    unsigned long long* out;     // ceil(m / 64) words
    unsigned long long* zeros;   // validity: += the zero bits among the m (null count); else nullptr
};

struct Utf8Args {
    Rows rows;
    const ColPtr* col;
    const unsigned* perm;
    unsigned m;
    unsigned* lens;              // [m + 1] k_sort_utf8_len: byte lengths, lens[m] = 0
    unsigned long long* total;   // k_sort_utf8_len: += bytes; k_sort_utf8_max: max length
    const int32_t* out_offsets;  // k_sort_utf8_copy: [m + 1]
    uint8_t* out_data;
};

// ---- sort.hip launchers (asynchronous on `st`)
hipError_t launch_word(const WordArgs& a, hipStream_t st);
// Stable sort of (words, perm) by bits [0, end_bit) into (words_out, perm_out); tmp == nullptr: *tmp_bytes only.
hipError_t radix_pass(void* tmp, size_t* tmp_bytes, const unsigned long long* words, unsigned long long* words_out,
                      const unsigned* perm, unsigned* perm_out, unsigned n, int end_bit, hipStream_t st);
// Radix select over words[0, n) of `bits` bits: the rows whose word is <= the k-th smallest, in row order, into
// cand; state->total = their count. hist: kSelectBins words; counts: ceil(n / kSelectRows) + 1 words.
hipError_t launch_select(const unsigned long long* words, unsigned n, int bits, unsigned long long k,
                         SelectState* state, unsigned* hist, unsigned* counts, void* tmp, size_t* tmp_bytes,
                         unsigned* cand, hipStream_t st);
hipError_t launch_gather(const GatherArgs& a, int width, hipStream_t st);
hipError_t launch_gather_bits(const BitsArgs& a, hipStream_t st);
hipError_t launch_utf8_max(const Utf8Args& a, hipStream_t st);  // over rows [0, rows.n), perm ignored
hipError_t launch_utf8_len(const Utf8Args& a, hipStream_t st);
// lens[0, m] -> offsets[0, m] (exclusive sums); tmp == nullptr: *tmp_bytes only.
hipError_t scan_offsets(void* tmp, size_t* tmp_bytes, const unsigned* lens, int32_t* offsets, unsigned m,
                        hipStream_t st);
hipError_t launch_utf8_copy(const Utf8Args& a, hipStream_t st);

}  // namespace srt
}  // namespace dfmi

#endif
