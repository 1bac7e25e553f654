// ORDER BY / LIMIT on the device: the fixed gfx950 kernels (sort.h has the
// protocol; sort.cpp drives them). Every kernel names a row by its global
// index over the input batches and resolves it through Rows / ColPtr; wave64
// throughout (a ballot is one 64-bit word of an output bitmap).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/dfmi.h"
#include "sort.h"
#include "sort_key.h"

namespace dfmi {
namespace srt {

typedef unsigned long long u64;
typedef unsigned char u8;

constexpr int kBlock = 256;

static inline unsigned grid_for(unsigned long long n, unsigned per_block = kBlock, unsigned cap = 1u << 16) {
    const unsigned long long g = (n + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Global row r -> (batch, physical slot of that batch's columns without the column's own offset).
__device__ __forceinline__ int locate(const Rows& R, unsigned r, unsigned& local) {
    int lo = 0, hi = R.nb;  // the last batch whose first row is <= r (0-row batches share a first row)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (R.prefix[mid] <= r) lo = mid; else hi = mid;
    }
    local = r - R.prefix[lo];
    return lo;
}

// Output row i's input row (no permutation: the input order).
__device__ __forceinline__ unsigned row_at(const unsigned* perm, unsigned long long i) {
    return perm ? perm[i] : (unsigned)i;
}

__device__ __forceinline__ bool bit_at(const u8* p, long long i) { return (p[i >> 3] >> (i & 7)) & 1; }

// Fixed-width value bits: Boolean 0/1, signed integers sign-extended,
// unsigned zero-extended, floats their raw bits (sort_key.h's input).
__device__ __forceinline__ u64 value_bits(int t, const void* v, long long i) {
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

// ------------------------------------------------------------- key words
__global__ __launch_bounds__(kBlock) void k_sort_word(const WordArgs A) {
    const int vbits = sort_value_bits(A.type);
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < A.n; i += gridDim.x * kBlock) {
        const unsigned r = A.perm ? A.perm[i] : i;
        if (!A.perm && A.perm_out) A.perm_out[i] = i;
        unsigned l;
        const ColPtr c = A.col[locate(A.rows, r, l)];
        const long long s = c.offset + l;
        const bool null = A.has_nulls && c.validity && !bit_at(c.validity, s);
        u64 w = 0;
        int bits = 64;
        switch (A.what) {
            case kWordNull:
                w = null;
                bits = 1;
                break;
            case kWordLength:
                w = null ? 0 : (u64)(unsigned)(c.offsets[s + 1] - c.offsets[s]);
                break;
            case kWordChunk:
            case kWordValue:
            case kWordSelect:
                if (A.type == DFMI_TYPE_UTF8) {
                    if (null) {
                        w = A.what == kWordSelect ? ~0ull : 0;
                        break;
                    }
                    const int o0 = c.offsets[s];
                    const unsigned len = (unsigned)(c.offsets[s + 1] - o0);
                    const u8* p = (const u8*)c.values + o0;
                    const unsigned b0 = 8u * (unsigned)A.chunk;
                    for (unsigned j = 0; j < 8; ++j) w = (w << 8) | (b0 + j < len ? p[b0 + j] : 0);
                } else if (A.null_above) {
                    w = null ? 1ull << vbits : sort_value_low(A.type, value_bits(A.type, c.values, s));
                    bits = vbits + 1;
                } else {
                    w = null ? (A.what == kWordSelect ? ~0ull : 0)
                             : sort_value_low(A.type, value_bits(A.type, c.values, s));
                    bits = vbits;
                }
                break;
        }
        if (!A.asc) w = bits == 64 ? ~w : (~w & ((1ull << bits) - 1));
        A.words[i] = w;
    }
}

// ----------------------------------------------------------- radix select
// Digit histogram of bits [lo, hi) over the rows whose bits above hi are the
// prefix found so far. Equal digits are first counted within the wave (the
// leading bits of a narrow key range are one digit for every row), what is
// left goes to LDS atomics, and each workgroup adds its non-zero bins once.
__global__ __launch_bounds__(kBlock) void k_sort_hist(const u64* words, unsigned n, const SelectState* st, int lo,
                                                      int hi, int first, unsigned* hist) {
    __shared__ unsigned bins[kSelectBins];
    for (int b = threadIdx.x; b < kSelectBins; b += kBlock) bins[b] = 0;
    __syncthreads();
    const u64 prefix = st->prefix;
    const unsigned dmask = (1u << (hi - lo)) - 1;
    const unsigned tiles = (n + kSelectRows - 1) / kSelectRows;
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        for (int k = 0; k < kSelectRows / kBlock; ++k) {
            const unsigned i = t * kSelectRows + k * kBlock + threadIdx.x;  // (n < 2^31: no overflow)
            bool live = false;
            unsigned d = 0;
            if (i < n) {
                const u64 w = words[i];
                live = first || (w >> hi) == (prefix >> hi);
                d = (unsigned)(w >> lo) & dmask;
            }
            for (int round = 0; round < 4; ++round) {  // wave-uniform trip count: every lane reaches the ballots
                const u64 any = __ballot(live);
                if (!any) break;
                const unsigned d0 = __shfl(d, __ffsll((long long)any) - 1);
                const u64 same = __ballot(live && d == d0);
                if (live && d == d0) {
                    if ((unsigned)(__ffsll((long long)same) - 1) == (threadIdx.x & 63)) atomicAdd(&bins[d0], __popcll(same));
                    live = false;
                }
            }
            if (live) atomicAdd(&bins[d], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kSelectBins; b += kBlock)
        if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

// The digit that holds rank k: one workgroup; the histogram is zeroed for the next pass.
__global__ __launch_bounds__(kBlock) void k_sort_pick(SelectState* st, unsigned* hist, int lo) {
    constexpr int kPer = kSelectBins / kBlock;
    __shared__ unsigned part[kBlock];
    unsigned mine[kPer];
    unsigned sum = 0;
    for (int j = 0; j < kPer; ++j) {
        mine[j] = hist[threadIdx.x * kPer + j];
        sum += mine[j];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    __shared__ int chunk;
    __shared__ u64 before;
    if (threadIdx.x == 0) {
        const u64 k = st->k;
        u64 cum = 0;
        int c = 0;
        while (c < kBlock - 1 && cum + part[c] < k) cum += part[c++];
        chunk = c;
        before = cum;
    }
    __syncthreads();
    if ((int)threadIdx.x == chunk) {
        const u64 k = st->k;
        u64 cum = before;
        int j = 0;
        while (j < kPer - 1 && cum + mine[j] < k) cum += mine[j++];
        st->prefix |= (u64)(unsigned)(chunk * kPer + j) << lo;
        st->k = k - cum;
    }
    for (int j = 0; j < kPer; ++j) hist[threadIdx.x * kPer + j] = 0;
}

// Rows of each tile whose word is <= the k-th word.
__global__ __launch_bounds__(kBlock) void k_sort_count(const u64* words, unsigned n, const SelectState* st,
                                                       unsigned* counts) {
    __shared__ unsigned wsum[kBlock / 64];
    const u64 T = st->prefix;
    const unsigned tiles = (n + kSelectRows - 1) / kSelectRows;
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        unsigned c = 0;
        for (int k = 0; k < kSelectRows / kBlock; ++k) {
            const unsigned i = t * kSelectRows + k * kBlock + threadIdx.x;
            c += __popcll(__ballot(i < n && words[i] <= T));
        }
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;  // (every lane of a wave holds the wave's count)
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned s = 0;
            for (int w = 0; w < kBlock / 64; ++w) s += wsum[w];
            counts[t] = s;
        }
        __syncthreads();
    }
}

// ... compacted in row order: ballot + prefix within the wave, wave totals through LDS.
__global__ __launch_bounds__(kBlock) void k_sort_select(const u64* words, unsigned n, SelectState* st,
                                                        const unsigned* offs, unsigned* cand) {
    __shared__ unsigned wsum[kBlock / 64];
    const u64 T = st->prefix;
    const unsigned tiles = (n + kSelectRows - 1) / kSelectRows;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->total = offs[tiles];
    for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
        unsigned base = offs[t];
        for (int k = 0; k < kSelectRows / kBlock; ++k) {
            const unsigned i = t * kSelectRows + k * kBlock + threadIdx.x;
            const bool keep = i < n && words[i] <= T;
            const u64 m = __ballot(keep);
            if (lane == 0) wsum[wave] = __popcll(m);
            __syncthreads();
            unsigned before = 0, all = 0;
            for (unsigned w = 0; w < kBlock / 64; ++w) {
                if (w < wave) before += wsum[w];
                all += wsum[w];
            }
            if (keep) cand[base + before + __popcll(m & ((1ull << lane) - 1))] = i;
            base += all;
            __syncthreads();
        }
    }
}

// ------------------------------------------------- gather by permutation
template <typename T>
__global__ __launch_bounds__(kBlock) void k_sort_gather(const GatherArgs A) {
    T* out = (T*)A.out;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < A.m; i += gridDim.x * kBlock) {
        unsigned l;
        const ColPtr c = A.col[locate(A.rows, row_at(A.perm, i), l)];
        out[i] = ((const T*)c.values)[c.offset + l];
    }
}

// Boolean values and validity bitmaps: one lane reads one source bit, the
// ballot is the output word (bits past m zero), lane 0 stores it.
__global__ __launch_bounds__(kBlock) void k_sort_gather_bits(const BitsArgs A) {
    __shared__ unsigned wzero[kBlock / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned nwords = (A.m + 63) / 64;
    const unsigned waves = gridDim.x * (kBlock / 64);
    unsigned zeros = 0;
    for (unsigned w = blockIdx.x * (kBlock / 64) + wave; w < nwords; w += waves) {
        const unsigned long long i = (unsigned long long)w * 64 + lane;
        bool bit = false;
        if (i < A.m) {
            unsigned l;
            const ColPtr c = A.col[locate(A.rows, row_at(A.perm, i), l)];
            const u8* src = A.validity ? c.validity : (const u8*)c.values;
            bit = src ? bit_at(src, c.offset + l) : true;
        }
        const u64 m = __ballot(bit);
        if (lane == 0) {
            A.out[w] = m;
            const unsigned in_range = A.m - w * 64 < 64 ? A.m - w * 64 : 64;
            zeros += in_range - __popcll(m);
        }
    }
    if (!A.zeros) return;
    if (lane == 0) wzero[wave] = zeros;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long z = 0;
        for (int w = 0; w < kBlock / 64; ++w) z += wzero[w];
        if (z) atomicAdd(A.zeros, z);
    }
}

// ------------------------------------------------------------------ Utf8
__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 x = __shfl_xor(v, o);
        v = x > v ? x : v;
    }
    return v;
}

// Longest string of the key column over every input row.
__global__ __launch_bounds__(kBlock) void k_sort_utf8_max(const Utf8Args A) {
    u64 mx = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < A.rows.n; i += gridDim.x * kBlock) {
        unsigned l;
        const ColPtr c = A.col[locate(A.rows, i, l)];
        const long long s = c.offset + l;
        const u64 len = (u64)(unsigned)(c.offsets[s + 1] - c.offsets[s]);
        mx = len > mx ? len : mx;
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(A.total, mx);
}

__global__ __launch_bounds__(kBlock) void k_sort_utf8_len(const Utf8Args A) {
    u64 sum = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i <= A.m; i += gridDim.x * kBlock) {
        unsigned len = 0;
        if (i < A.m) {
            unsigned l;
            const ColPtr c = A.col[locate(A.rows, row_at(A.perm, i), l)];
            const long long s = c.offset + l;
            len = (unsigned)(c.offsets[s + 1] - c.offsets[s]);
        }
        A.lens[i] = len;
        sum += len;
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(A.total, sum);
}

// One wave per 64 output rows: a short string is copied by its own lane, a
// longer one by the whole wave, 64 consecutive bytes per step.
__global__ __launch_bounds__(kBlock) void k_sort_utf8_copy(const Utf8Args A) {
    const unsigned lane = threadIdx.x & 63;
    const unsigned groups = (A.m + 63) / 64;
    const unsigned waves = gridDim.x * (kBlock / 64);
    for (unsigned g = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); g < groups; g += waves) {
        const unsigned long long i = (unsigned long long)g * 64 + lane;
        unsigned len = 0;
        u64 src = 0;
        unsigned dst = 0;
        if (i < A.m) {
            unsigned l;
            const ColPtr c = A.col[locate(A.rows, row_at(A.perm, i), l)];
            const long long s = c.offset + l;
            const int o0 = c.offsets[s];
            len = (unsigned)(c.offsets[s + 1] - o0);
            src = (u64)(uintptr_t)((const u8*)c.values + o0);
            dst = (unsigned)A.out_offsets[i];
        }
        if (len <= kShortString)
            for (unsigned j = 0; j < len; ++j) A.out_data[dst + j] = ((const u8*)(uintptr_t)src)[j];
        u64 big = __ballot(len > kShortString);
        while (big) {  // (wave-uniform)
            const int L = __ffsll((long long)big) - 1;
            big &= big - 1;
            const u8* sp = (const u8*)(uintptr_t)__shfl(src, L);
            const unsigned dp = __shfl(dst, L), ln = __shfl(len, L);
            for (unsigned j = lane; j < ln; j += 64) A.out_data[dp + j] = sp[j];
        }
    }
}

// ---------------------------------------------------------------- launchers
hipError_t launch_word(const WordArgs& a, hipStream_t st) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(k_sort_word, dim3(grid_for(a.n)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t radix_pass(void* tmp, size_t* tmp_bytes, const u64* words, u64* words_out, const unsigned* perm,
                      unsigned* perm_out, unsigned n, int end_bit, hipStream_t st) {
    return rocprim::radix_sort_pairs(tmp, *tmp_bytes, words, words_out, perm, perm_out, (size_t)n, 0u,
                                     (unsigned)end_bit, st);
}

hipError_t launch_select(const u64* words, unsigned n, int bits, u64 k, SelectState* state, unsigned* hist,
                         unsigned* counts, void* tmp, size_t* tmp_bytes, unsigned* cand, hipStream_t st) {
    const unsigned tiles = (n + kSelectRows - 1) / kSelectRows;
    unsigned* offs = counts + tiles + 1;
    if (!tmp) return rocprim::exclusive_scan(nullptr, *tmp_bytes, counts, offs, 0u, (size_t)tiles + 1,
                                             rocprim::plus<unsigned>(), st);
    const SelectState init{0, k, 0, 0};
    hipError_t e = hipMemcpyAsync(state, &init, sizeof init, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(hist, 0, kSelectBins * sizeof(unsigned), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(counts, 0, ((size_t)tiles + 1) * sizeof(unsigned), st)) != hipSuccess) return e;
    const unsigned g = grid_for(tiles, 1, 1024);
    for (int hi = bits; hi > 0;) {
        const int lo = hi > kSelectBits ? hi - kSelectBits : 0;
        hipLaunchKernelGGL(k_sort_hist, dim3(g), dim3(kBlock), 0, st, words, n, (const SelectState*)state, lo, hi,
                           hi == bits ? 1 : 0, hist);
        hipLaunchKernelGGL(k_sort_pick, dim3(1), dim3(kBlock), 0, st, state, hist, lo);
        hi = lo;
    }
    hipLaunchKernelGGL(k_sort_count, dim3(g), dim3(kBlock), 0, st, words, n, (const SelectState*)state, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::exclusive_scan(tmp, *tmp_bytes, counts, offs, 0u, (size_t)tiles + 1, rocprim::plus<unsigned>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sort_select, dim3(g), dim3(kBlock), 0, st, words, n, state, (const unsigned*)offs, cand);
    return hipGetLastError();
}

hipError_t launch_gather(const GatherArgs& a, int width, hipStream_t st) {
    if (!a.m) return hipSuccess;
    const dim3 g(grid_for(a.m)), b(kBlock);
    switch (width) {
        case 1: hipLaunchKernelGGL(k_sort_gather<unsigned char>, g, b, 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_sort_gather<unsigned short>, g, b, 0, st, a); break;
        case 4: hipLaunchKernelGGL(k_sort_gather<unsigned>, g, b, 0, st, a); break;
        case 8: hipLaunchKernelGGL(k_sort_gather<u64>, g, b, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_gather_bits(const BitsArgs& a, hipStream_t st) {
    if (!a.m) return hipSuccess;
    hipLaunchKernelGGL(k_sort_gather_bits, dim3(grid_for((a.m + 63) / 64, kBlock / 64, 2048)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_utf8_max(const Utf8Args& a, hipStream_t st) {
    if (!a.rows.n) return hipSuccess;
    hipLaunchKernelGGL(k_sort_utf8_max, dim3(grid_for(a.rows.n, kBlock, 2048)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_utf8_len(const Utf8Args& a, hipStream_t st) {
    hipLaunchKernelGGL(k_sort_utf8_len, dim3(grid_for((u64)a.m + 1, kBlock, 2048)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t scan_offsets(void* tmp, size_t* tmp_bytes, const unsigned* lens, int32_t* offsets, unsigned m,
                        hipStream_t st) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, lens, (unsigned*)offsets, 0u, (size_t)m + 1,
                                   rocprim::plus<unsigned>(), st);
}

hipError_t launch_utf8_copy(const Utf8Args& a, hipStream_t st) {
    if (!a.m) return hipSuccess;
    hipLaunchKernelGGL(k_sort_utf8_copy, dim3(grid_for((a.m + 63) / 64, kBlock / 64)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace srt
}  // namespace dfmi
