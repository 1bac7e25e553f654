// CSV output on the device: the fixed gfx950 kernels (csv_write.h has the
// protocol, csv_field.h the field rules, format_core.h the numbers' bytes;
// csv_write.cpp drives them). wave64 throughout.
//
//   k_csv_quote_scan  over the BYTES of every Utf8 column, 16 per lane and load,
//                     coalesced: a lane that meets '"', ',', '\n' or '\r' finds
//                     the byte's row by a search over the column's offsets and
//                     marks that row's quote word (special bytes are rare, so
//                     the searches and the atomics are too).
//   k_csv_measure     one row per lane, a loop over the batch's columns: the
//                     record's byte length into its slot, per batch the bytes.
//   (scan)            rocprim's exclusive scan over the slots.
//   k_csv_write       a 64-row slice's records are one contiguous span of the
//                     stream: the lanes lay their records into a per-wave LDS
//                     image at the span's alignment and the wave stores it as
//                     aligned 32-bit words; only the two edge words, which the
//                     neighbouring slices share, go out bytewise. A span longer
//                     than the image (long strings, long floats) is stored per
//                     lane.
// The float digits are computed in both passes (DESIGN.md §6 "CSV output").
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dfmi.h"
#include "csv_field.h"
#include "csv_write.h"
#include "format_core.h"

namespace dfmi {
namespace csvk {

typedef unsigned long long u64;
typedef unsigned char u8;

__device__ __forceinline__ bool bit_at(const u8* p, unsigned i) { return (p[i >> 3] >> (i & 7)) & 1; }

// Boolean 0 / 1, signed integers sign-extended, unsigned zero-extended, floats their raw bits.
__device__ __forceinline__ u64 value_bits(int t, const void* v, unsigned i) {
    switch (t) {
        case 1: return bit_at((const u8*)v, i);
        case 2: return (u64)(long long)((const signed char*)v)[i];
        case 3: return (u64)(long long)((const short*)v)[i];
        case 4: return (u64)(long long)((const int*)v)[i];
        case 6: return (u64)((const u8*)v)[i];
        case 7: return (u64)((const unsigned short*)v)[i];
        case 8: case 10: return (u64)((const unsigned*)v)[i];
        case 5: case 9: case 11: return ((const u64*)v)[i];
        default: return 0;
    }
}

// The batch of tile t: the last one whose first tile is <= t (a batch without rows has no tile).
__device__ __forceinline__ int batch_of(const Args& A, unsigned t) {
    int lo = 0, hi = A.nbatches;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.batches[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Every job is one Utf8 column of one batch; its byte range [offsets[0], offsets[n]) is cut at 16-byte
// addresses into steps of kTileRows * kScanBytes bytes, dealt round to the workgroups (a job's first step
// goes to workgroup job % grid, so many small batches spread out). Nothing below offsets[0] or past
// offsets[n] is read: the 16 bytes that straddle an end are read bytewise.
__global__ __launch_bounds__(kTileRows) void k_csv_quote_scan(const Args A) {
    const int jobs = A.nbatches * A.nutf8;
    constexpr unsigned kStep = (unsigned)kTileRows * kScanBytes;
    for (int job = 0; job < jobs; ++job) {
        const int b = job / A.nutf8;
        const unsigned n = A.batches[b].n;
        if (!n) continue;
        const Col C = A.cols[(size_t)b * A.ncols + A.utf8_cols[job % A.nutf8]];
        const u8* base = (const u8*)C.values;
        const int32_t lo = C.offsets[0], hi = C.offsets[n];
        if (hi <= lo) continue;
        const u8* beg = base + lo;
        const u8* end = base + hi;
        const u8* first = (const u8*)((uintptr_t)beg & ~(uintptr_t)(kScanBytes - 1));
        const size_t steps = ((size_t)(end - first) + kStep - 1) / kStep;
        for (size_t s = (blockIdx.x + gridDim.x - (unsigned)job % gridDim.x) % gridDim.x; s < steps; s += gridDim.x) {
            const u8* p = first + s * kStep + (size_t)threadIdx.x * kScanBytes;
            if (p >= end || p + kScanBytes <= beg) continue;
            unsigned w[4];
            if (p >= beg && p + kScanBytes <= end) {
                const uint4 v = *(const uint4*)p;
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            } else {
                for (int i = 0; i < 4; ++i) {
                    unsigned x = 0;
                    for (int k = 0; k < 4; ++k) {
                        const u8* q = p + i * 4 + k;
                        if (q >= beg && q < end) x |= (unsigned)*q << (8 * k);
                    }
                    w[i] = x;  // (a byte outside the range reads as 0, which is no special byte)
                }
            }
            for (int i = 0; i < 4; ++i) {
                unsigned m = csv::special_mask(w[i]);
                while (m) {
                    const int k = (__ffs((int)m) - 1) >> 3;
                    m &= m - 1;
                    const int32_t pos = (int32_t)(p + i * 4 + k - base);
                    unsigned r0 = 0, r1 = n;  // offsets[r0] <= pos < offsets[r1]
                    while (r1 - r0 > 1) {
                        const unsigned mid = (r0 + r1) >> 1;
                        if (C.offsets[mid] <= pos) r0 = mid; else r1 = mid;
                    }
                    if (((w[i] >> (8 * k)) & 0xffu) == '"') atomicAdd(&C.quote[r0], 1u);
                    else atomicOr(&C.quote[r0], kQuoteFlag);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kTileRows) void k_csv_measure(const Args A) {
    const unsigned lane = threadIdx.x & 63;
    int cur = -1;  // the batch the wave's sum belongs to
    u64 bytes = 0;
    auto flush = [&]() {
        if (cur >= 0 && lane == 0 && bytes) atomicAdd(&A.totals[cur], bytes);
    };
    for (unsigned t = blockIdx.x; t < A.tiles; t += gridDim.x) {
        const int b = batch_of(A, t);
        if (b != cur) {
            flush();
            cur = b, bytes = 0;
        }
        const Batch B = A.batches[b];
        const unsigned row = (t - B.tile0) * kTileRows + threadIdx.x;
        u64 len = 0;
        if (row < B.n) {
            const Col* cols = A.cols + (size_t)b * A.ncols;
            for (int c = 0; c < A.ncols; ++c) {
                const Col& C = cols[c];
                if (C.validity && !bit_at(C.validity, row)) continue;  // a null: an empty field
                if (C.type == DFMI_TYPE_UTF8) {
                    const unsigned q = C.quote[row];
                    len += csv::utf8_length((u64)(unsigned)(C.offsets[row + 1] - C.offsets[row]), q & ~kQuoteFlag, q != 0);
                } else {
                    const u64 bits = value_bits(C.type, C.values, row);
                    if (C.type >= DFMI_TYPE_FLOAT32) {
                        fmt::Dec d;
                        fmt::dec_from_value(d, C.type, bits);
                        len += (u64)fmt::fmt_length(d);
                    } else {
                        len += (u64)fmt::fmt_length_int(C.type, bits);
                    }
                }
            }
            if (csv::empty_record(A.ncols, len)) len = 2;
            len += (u64)A.ncols;  // the separators and the newline
        }
        // (a record of 2^32 bytes or more: its batch total says so, and the driver stops before the scan)
        A.lens[(size_t)t * kTileRows + threadIdx.x] = len > 0xffffffffull ? 0xffffffffu : (unsigned)len;
        const u64 sum = wave_sum(len);
        if (lane == 0) bytes += sum;
    }
    flush();
}

// One record at p (LDS image or the stream): exactly the bytes k_csv_measure counted.
__device__ __forceinline__ void write_record(u8* p, const Args& A, int b, unsigned row) {
    const Col* cols = A.cols + (size_t)b * A.ncols;
    u8* q = p;
    for (int c = 0; c < A.ncols; ++c) {
        if (c) *q++ = ',';
        const Col& C = cols[c];
        if (C.validity && !bit_at(C.validity, row)) continue;
        if (C.type == DFMI_TYPE_UTF8) {
            const int32_t o = C.offsets[row];
            q += csv::copy_field(q, (const u8*)C.values + o, (u64)(unsigned)(C.offsets[row + 1] - o), C.quote[row] != 0);
        } else {
            fmt::Dec d;
            fmt::dec_from_value(d, C.type, value_bits(C.type, C.values, row));
            const int n = fmt::fmt_length(d);
            for (int j = 0; j < n; ++j) q[j] = fmt::fmt_byte(d, j);
            q += n;
        }
    }
    if (csv::empty_record(A.ncols, (u64)(q - p))) {
        *q++ = '"';
        *q++ = '"';
    }
    *q = '\n';
}

__global__ __launch_bounds__(kTileRows) void k_csv_write(const Args A) {
    __shared__ __attribute__((aligned(16))) u8 stage[kTileRows / 64][kImageBytes + 8];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u8* img = stage[wave];
    for (unsigned t = blockIdx.x; t < A.tiles; t += gridDim.x) {  // (every branch up to the barrier is uniform per workgroup)
        const int b = batch_of(A, t);
        const Batch B = A.batches[b];
        const unsigned row = (t - B.tile0) * kTileRows + threadIdx.x;
        const size_t g = (size_t)t * kTileRows + threadIdx.x;
        const unsigned o0 = A.sums[g], o1 = A.sums[g + 1];  // (a row past the end has length 0)
        const bool in = row < B.n;
        // the slice's span [s0, s1) of the stream
        const unsigned s0 = __shfl(o0, 0), s1 = __shfl(o1, 63);
        const unsigned span = s1 - s0;
        u8* dst = A.data + s0;
        const unsigned a0 = (unsigned)((uintptr_t)dst & 3);
        const bool staged = a0 + span <= (unsigned)kImageBytes;  // (uniform per wave)
        if (in) {
            if (staged) write_record(img + a0 + (o0 - s0), A, b, row);
            else write_record(A.data + o0, A, b, row);
        }
        __syncthreads();
        if (staged && span) {
            u8* dstb = dst - a0;  // 4-byte aligned
            const unsigned end = a0 + span, nw = (end + 3) >> 2;
            for (unsigned w = lane; w < nw; w += 64) {
                const unsigned lo = w << 2;
                if (lo >= a0 && lo + 4 <= end) {
                    *(unsigned*)(dstb + lo) = *(const unsigned*)(img + lo);
                } else {
                    for (unsigned k = lo; k < lo + 4; ++k)
                        if (k >= a0 && k < end) dstb[k] = img[k];
                }
            }
        }
        __syncthreads();
    }
}

hipError_t launch_quote_scan(const Args& a, unsigned grid, hipStream_t st) {
    if (!a.tiles || !a.nutf8) return hipSuccess;
    hipLaunchKernelGGL(k_csv_quote_scan, dim3(grid), dim3(kTileRows), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_measure(const Args& a, unsigned grid, hipStream_t st) {
    if (!a.tiles) return hipSuccess;
    hipLaunchKernelGGL(k_csv_measure, dim3(grid), dim3(kTileRows), 0, st, a);
    return hipGetLastError();
}

hipError_t scan_lengths(void* tmp, size_t* tmp_bytes, const Args& a, hipStream_t st) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, a.lens, a.sums, 0u, (size_t)a.tiles * kTileRows + 1,
                                   rocprim::plus<unsigned>(), st);
}

hipError_t launch_write(const Args& a, unsigned grid, hipStream_t st) {
    if (!a.tiles) return hipSuccess;
    hipLaunchKernelGGL(k_csv_write, dim3(grid), dim3(kTileRows), 0, st, a);
    return hipGetLastError();
}

}  // namespace csvk
}  // namespace dfmi
