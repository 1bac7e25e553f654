// CSV output (DFMI_FLAG_EXT_CSV_WRITE, DESIGN.md §4 "CSV output"): the field
// rules -- which bytes force quotes, a Utf8 field's encoded length, the copy
// that doubles quotes, the one-column empty record -- as plain C++ with no
// library call and no wave intrinsic: one text for the device kernels
// (csv_write.hip), for dfmi_csv_header on the host and for the host driver
// that runs it under ASan + UBSan (tests/native/csv_write_driver.cpp), in the
// way format_core.h is shared. Numbers and Booleans are format_core.h's bytes.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef DFMI_HD
#define DFMI_HD __host__ __device__
#endif
#else
#ifndef DFMI_HD
#define DFMI_HD
#endif
#endif

namespace dfmi {
namespace csv {

// A byte that forces its field into quotes: the reader would end the field (','),
// end the record ('\n', and '\r' before it is dropped) or open a quoted field ('"').
DFMI_HD inline bool special_byte(unsigned char b) { return b == '"' || b == ',' || b == '\n' || b == '\r'; }

// ... of the four bytes of a little-endian word, without a branch per byte: bit 7 of
// byte k of the result is set exactly when byte k of w is special.
DFMI_HD inline unsigned zero_bytes(unsigned x) {  // bit 7 of every zero byte of x, exactly (no carry between bytes)
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
DFMI_HD inline unsigned special_mask(unsigned w) {
    return zero_bytes(w ^ 0x22222222u) | zero_bytes(w ^ 0x2c2c2c2cu) | zero_bytes(w ^ 0x0a0a0a0au) |
           zero_bytes(w ^ 0x0d0d0d0du);
}

// Encoded bytes of a Utf8 field of `raw` bytes, `quotes` of them '"'.
DFMI_HD inline unsigned long long utf8_length(unsigned long long raw, unsigned long long quotes, bool needs_quotes) {
    return needs_quotes ? raw + quotes + 2 : raw;
}

// A record of one column whose only field is empty is written as `""`: the reader
// skips an empty record, and reads `""` as the empty string / a numeric null.
DFMI_HD inline bool empty_record(int num_columns, unsigned long long field_length) {
    return num_columns == 1 && field_length == 0;
}

// The field's bytes at dst (utf8_length of them): returns the count.
DFMI_HD inline unsigned long long copy_field(unsigned char* dst, const unsigned char* src, unsigned long long raw,
                                             bool needs_quotes) {
    if (!needs_quotes) {
        for (unsigned long long i = 0; i < raw; ++i) dst[i] = src[i];
        return raw;
    }
    unsigned long long o = 0;
    dst[o++] = '"';
    for (unsigned long long i = 0; i < raw; ++i) {
        const unsigned char b = src[i];
        dst[o++] = b;
        if (b == '"') dst[o++] = '"';
    }
    dst[o++] = '"';
    return o;
}

// A field on the host, where nothing has counted its bytes yet: its quote count and whether it needs quotes.
inline void scan_field(const unsigned char* src, unsigned long long raw, unsigned long long* quotes, bool* needs_quotes) {
    unsigned long long q = 0;
    bool need = false;
    for (unsigned long long i = 0; i < raw; ++i) {
        q += src[i] == '"';
        need |= special_byte(src[i]);
    }
    *quotes = q;
    *needs_quotes = need;
}

}  // namespace csv
}  // namespace dfmi
