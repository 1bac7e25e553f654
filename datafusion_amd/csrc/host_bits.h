// Bit-level splicing of LSB-first bitmaps: the chunk pipeline
// (host_chunks.cpp) concatenates each chunk's Boolean values and validity at
// a row position that is seldom a byte boundary. Host only.
#pragma once
#include <cstdint>
#include <cstring>

namespace dfmi {
namespace host {

inline uint64_t ld64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
inline void st64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }

// Write bits [0, n) of LSB-first bitmap src at bit position pos of dst.
// Bits of dst below pos are kept; bits past pos + n may be overwritten (the
// next chunk's append, or finish_bitmap, owns them). src holds >= ceil(n/8)
// bytes; dst >= ceil((pos + n)/8) bytes plus 8 of slack.
inline void append_bits(uint8_t* dst, int64_t pos, const uint8_t* src, int64_t n) {
    if (n <= 0) return;
    uint8_t* d = dst + (pos >> 3);
    const int sh = (int)(pos & 7);
    const int64_t nb = (n + 7) >> 3;
    if (!sh) {
        memcpy(d, src, (size_t)nb);
        return;
    }
    uint8_t carry = d[0] & (uint8_t)((1u << sh) - 1);
    int64_t i = 0;
    for (; i + 8 <= nb; i += 8) {
        const uint64_t v = ld64(src + i);
        st64(d + i, (v << sh) | carry);
        carry = (uint8_t)(v >> (64 - sh));
    }
    for (; i < nb; ++i) {
        const uint8_t b = src[i];
        d[i] = (uint8_t)(b << sh) | carry;
        carry = (uint8_t)(b >> (8 - sh));
    }
    d[nb] = carry;
}

// Set bits [pos, pos + n) (a chunk whose result holds no nulls).
inline void append_ones(uint8_t* dst, int64_t pos, int64_t n) {
    if (n <= 0) return;
    int64_t p = pos, e = pos + n;
    while (p < e && (p & 7)) {
        dst[p >> 3] |= (uint8_t)(1u << (p & 7));
        ++p;
    }
    if (p < e) {
        const int64_t full = (e - p) >> 3;
        memset(dst + (p >> 3), 0xff, (size_t)full);
        p += full * 8;
        if (p < e) dst[p >> 3] = (uint8_t)((1u << (e - p)) - 1);
    }
}

// Zero the bits of the last byte past n (arrow's bitmaps carry no garbage).
inline void finish_bitmap(uint8_t* b, int64_t n) {
    if (n & 7) b[n >> 3] &= (uint8_t)((1u << (n & 7)) - 1);
}

}  // namespace host
}  // namespace dfmi
