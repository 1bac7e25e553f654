// The order-preserving unsigned encoding of a key value (DESIGN.md §2 key
// order), shared by GROUP BY's device emission (groupby.hip) and ORDER BY
// (sort.hip): comparing the words as unsigned integers compares the values.
#pragma once
#include <hip/hip_runtime.h>

namespace dfmi {

// `bits`: Boolean 0/1, signed integers sign-extended, unsigned zero-extended,
// floats their raw bits. false < true, integers numerically, floats by IEEE
// 754 totalOrder (one position per bit pattern).
__device__ __forceinline__ unsigned long long sort_value(int t, unsigned long long bits) {
    switch (t) {
        case 11: return (bits >> 63) ? ~bits : (bits | (1ull << 63));  // Float64: totalOrder
        case 10: {
            const unsigned b = (unsigned)bits;
            return (unsigned long long)((b >> 31) ? ~b : (b | 0x80000000u));
        }
        case 2: case 3: case 4: case 5: return bits ^ (1ull << 63);  // signed: sign-extended bits
        default: return bits;  // unsigned, Boolean
    }
}

// Bits of the type's values: the width of sort_value_low's word.
__host__ __device__ __forceinline__ int sort_value_bits(int t) {
    switch (t) {
        case 1: return 1;
        case 2: case 6: return 8;
        case 3: case 7: return 16;
        case 4: case 8: case 10: return 32;
        default: return 64;
    }
}

// sort_value in sort_value_bits(t) bits: a narrow signed integer's bias moves
// from bit 63 to its own sign bit, every other type's word already fits.
__device__ __forceinline__ unsigned long long sort_value_low(int t, unsigned long long bits) {
    const unsigned long long w = sort_value(t, bits);
    switch (t) {
        case 2: return (w ^ (1ull << 63) ^ (1ull << 7)) & 0xffull;
        case 3: return (w ^ (1ull << 63) ^ (1ull << 15)) & 0xffffull;
        case 4: return (w ^ (1ull << 63) ^ (1ull << 31)) & 0xffffffffull;
        default: return w;
    }
}

}  // namespace dfmi
