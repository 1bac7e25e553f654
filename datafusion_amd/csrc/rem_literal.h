// Host half of the literal-divisor remainder (jit_skeleton.hip irem_lit,
// DFMI_FLAG_EXT_MODULUS): the reciprocal the kernel multiplies by. Plain
// C++, no HIP: tests/native/modulus_driver.cpp includes it too.
#pragma once
#include <cstdint>

namespace dfmi {

// floor((2^N - 1) / |d|) for the literal d held in `bits` (sign / zero
// extended or not: only the low `width` bytes count), N = 32 for operands of
// up to 4 bytes and 64 for 8-byte operands; 0 for d = 0. |iN::MIN| fits the
// unsigned type.
inline uint64_t rem_reciprocal(int width, bool is_signed, uint64_t bits) {
    const int sh = 64 - 8 * width;
    uint64_t ad = (bits << sh) >> sh;
    if (is_signed) {
        const int64_t d = (int64_t)(bits << sh) >> sh;
        if (d < 0) ad = 0 - (uint64_t)d;
    }
    if (ad == 0) return 0;
    return (width == 8 ? ~0ull : 0xFFFFFFFFull) / ad;
}

}  // namespace dfmi
