// CAST to Utf8 on the device: the fixed gfx950 kernels (format.h has the
// protocol, format_core.h the formatting; format.cpp drives them). wave64
// throughout: a ballot is one 64-bit word of the output validity.
//
//   k_format_measure  one row per lane, coalesced typed loads: the row's byte
//                     length into its slot, the validity word of each 64-row
//                     slice, per column the bytes and the nulls.
//   (scan)            rocprim's exclusive scan over the slots.
//   k_format_write    the offsets, then the bytes: a slice's output span is
//                     contiguous, so its rows are laid into an LDS image at
//                     the span's alignment and stored as aligned 32-bit words,
//                     lane after lane; only the two edge words, which the
//                     neighbouring slices share, go out bytewise. A span longer
//                     than the image (long float strings) is stored per lane.
// The float digits are computed in both passes (DESIGN.md §6 "CAST to Utf8").
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dfmi.h"
#include "format.h"
#include "format_core.h"

namespace dfmi {
namespace fmtk {

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

// The column of tile t: the last one whose first tile is <= t (a column without rows has no tile).
__device__ __forceinline__ int column_of(const Args& A, unsigned t) {
    int lo = 0, hi = A.ncols;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.cols[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kTileRows) void k_format_measure(const Args A) {
    const unsigned lane = threadIdx.x & 63;
    int cur = -1;          // the column the wave's sums belong to
    u64 bytes = 0, nulls = 0, exact = 0, decimal = 0, integer = 0;
    auto flush = [&]() {
        if (cur < 0 || lane != 0) return;
        if (bytes) atomicAdd(&A.totals[2 * cur], bytes);
        if (nulls) atomicAdd(&A.totals[2 * cur + 1], nulls);
    };
    for (unsigned t = blockIdx.x; t < A.tiles; t += gridDim.x) {
        const int c = column_of(A, t);
        if (c != cur) {
            flush();
            cur = c, bytes = 0, nulls = 0;
        }
        const Col C = A.cols[c];
        const unsigned row = (t - C.tile0) * kTileRows + threadIdx.x;
        const bool in = row < C.n;
        const bool valid = in && (!C.validity || bit_at(C.validity, row));
        unsigned len = 0;
        if (valid) {
            const u64 bits = value_bits(C.type, C.values, row);
            if (C.type >= DFMI_TYPE_FLOAT32) {
                fmt::Dec d;
                const int path = fmt::dec_from_value(d, C.type, bits);
                len = (unsigned)fmt::fmt_length(d);
                exact += path == fmt::kPathExact, decimal += path == fmt::kPathDecimal;
                integer += path == fmt::kPathInteger;
            } else {
                len = (unsigned)fmt::fmt_length_int(C.type, bits);
            }
        }
        A.lens[(size_t)t * kTileRows + threadIdx.x] = len;
        const u64 sum = wave_sum(len);
        const u64 m = __ballot(valid);
        const unsigned first = row - lane;  // the slice's first row
        if (lane == 0) {
            bytes += sum;
            if (C.out_validity && first < C.n) {
                C.out_validity[first >> 6] = m;
                const unsigned in_range = C.n - first < 64 ? C.n - first : 64;
                nulls += in_range - __popcll(m);
            }
        }
    }
    flush();
    if (A.paths) {
        exact = wave_sum(exact), decimal = wave_sum(decimal), integer = wave_sum(integer);
        if (lane == 0) {
            if (integer) atomicAdd(&A.paths[fmt::kPathInteger], integer);
            if (decimal) atomicAdd(&A.paths[fmt::kPathDecimal], decimal);
            if (exact) atomicAdd(&A.paths[fmt::kPathExact], exact);
        }
    }
}

__global__ __launch_bounds__(kTileRows) void k_format_write(const Args A) {
    __shared__ __attribute__((aligned(16))) u8 stage[kTileRows / 64][kStageBytes + 8];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u8* img = stage[wave];
    for (unsigned t = blockIdx.x; t < A.tiles; t += gridDim.x) {  // (every branch up to the barrier is uniform per workgroup)
        const Col C = A.cols[column_of(A, t)];
        const unsigned row = (t - C.tile0) * kTileRows + threadIdx.x;
        const size_t g = (size_t)t * kTileRows + threadIdx.x;
        const unsigned base = A.sums[(size_t)C.tile0 * kTileRows];
        const unsigned o0 = A.sums[g] - base, o1 = A.sums[g + 1] - base;
        const bool in = row < C.n;
        if (in) {
            C.offsets[row] = (int32_t)o0;
            if (row == C.n - 1) C.offsets[C.n] = (int32_t)o1;
        }
        if (!C.data) continue;  // measure only
        const unsigned len = in ? o1 - o0 : 0;  // (a null row's and a row's past the end: 0)
        fmt::Dec d;
        if (len) fmt::dec_from_value(d, C.type, value_bits(C.type, C.values, row));
        // the slice's span [s0, s1) of the column's bytes
        const unsigned s0 = __shfl(o0, 0), s1 = __shfl(in ? o1 : o0, 63);
        const unsigned span = s1 - s0;
        u8* dst = C.data + s0;
        const unsigned a0 = (unsigned)((uintptr_t)dst & 3);
        const bool staged = a0 + span <= (unsigned)kStageBytes;  // (uniform per wave)
        if (staged) {
            u8* p = img + a0 + (o0 - s0);
            for (unsigned j = 0; j < len; ++j) p[j] = fmt::fmt_byte(d, (int)j);
        } else {
            u8* p = C.data + o0;
            for (unsigned j = 0; j < len; ++j) p[j] = fmt::fmt_byte(d, (int)j);
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
                    for (unsigned b = lo; b < lo + 4; ++b)
                        if (b >= a0 && b < end) dstb[b] = img[b];
                }
            }
        }
        __syncthreads();
    }
}

hipError_t launch_measure(const Args& a, unsigned grid, hipStream_t st) {
    if (!a.tiles) return hipSuccess;
    hipLaunchKernelGGL(k_format_measure, dim3(grid), dim3(kTileRows), 0, st, a);
    return hipGetLastError();
}

hipError_t scan_lengths(void* tmp, size_t* tmp_bytes, const Args& a, hipStream_t st) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, a.lens, a.sums, 0u, (size_t)a.tiles * kTileRows + 1,
                                   rocprim::plus<unsigned>(), st);
}

hipError_t launch_write(const Args& a, unsigned grid, hipStream_t st) {
    if (!a.tiles) return hipSuccess;
    hipLaunchKernelGGL(k_format_write, dim3(grid), dim3(kTileRows), 0, st, a);
    return hipGetLastError();
}

}  // namespace fmtk
}  // namespace dfmi
