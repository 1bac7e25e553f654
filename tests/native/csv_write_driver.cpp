// Host-code driver (TEST INFRASTRUCTURE) of the CSV field rules behind
// DFMI_FLAG_EXT_CSV_WRITE. Built with AddressSanitizer +
// UndefinedBehaviorSanitizer and run by tests/test_csv_write_cpu.py; it
// includes csrc/csv_field.h and csrc/format_core.h themselves: the text the
// device compiles is the text run here, in the order the kernels run it. Every
// record is measured first (fmt_length / fmt_length_int for numbers,
// utf8_length from a field's quote count and needs-quotes bit, the one-column
// empty rule), then written into a heap block of exactly that length, so a
// disagreement between the two passes is a sanitizer finding. special_mask is
// checked against special_byte on every word of every string on the way.
//
// argv[1]: the records (little-endian): int32 ncols, int32 types[ncols] (dfmi_type),
//          int64 nrows, then per row and column: uint8 valid, and for Utf8 int32 len + bytes,
//          else uint64 bits (signed integers sign-extended, floats their raw bits).
// argv[2]: the encoded stream. Exit 0 and a closing "clean" line on stdout = no finding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "csv_field.h"
#include "format_core.h"

using namespace dfmi;

namespace {

struct Field {
    bool valid = false;
    uint64_t bits = 0;
    std::vector<unsigned char> str;
};

template <typename T>
T get(FILE* f) {
    T v;
    if (fread(&v, sizeof v, 1, f) != 1) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return v;
}

long mask_mismatches(const std::vector<unsigned char>& s) {
    long bad = 0;
    for (size_t i = 0; i < s.size(); i += 4) {
        unsigned w = 0;
        for (size_t k = 0; k < 4 && i + k < s.size(); ++k) w |= (unsigned)s[i + k] << (8 * k);
        const unsigned m = csv::special_mask(w);
        for (size_t k = 0; k < 4; ++k) {
            const bool want = i + k < s.size() && csv::special_byte(s[i + k]);
            bad += (((m >> (8 * k + 7)) & 1u) != 0) != want;
            bad += ((m >> (8 * k)) & 0x7fu) != 0;  // (only bit 7 of a byte is ever set)
        }
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int ncols = get<int32_t>(in);
    std::vector<int> types((size_t)ncols);
    for (int c = 0; c < ncols; ++c) types[c] = get<int32_t>(in);
    const long long nrows = get<int64_t>(in);
    long bad_mask = 0, bad_len = 0;
    unsigned long long total = 0;
    std::vector<Field> row((size_t)ncols);
    for (long long r = 0; r < nrows; ++r) {
        for (int c = 0; c < ncols; ++c) {
            Field& f = row[c];
            f.valid = get<uint8_t>(in) != 0;
            if (types[c] == 12) {
                const int32_t n = get<int32_t>(in);
                f.str.resize((size_t)n);
                if (n && fread(f.str.data(), 1, (size_t)n, in) != (size_t)n) return 2;
                bad_mask += mask_mismatches(f.str);
            } else {
                f.bits = get<uint64_t>(in);
            }
        }
        // ---- measure (k_csv_measure)
        unsigned long long len = 0;
        std::vector<unsigned long long> quotes((size_t)ncols, 0);
        std::vector<char> quoted((size_t)ncols, 0);
        for (int c = 0; c < ncols; ++c) {
            const Field& f = row[c];
            if (!f.valid) continue;
            if (types[c] == 12) {
                bool q = false;
                csv::scan_field(f.str.data(), f.str.size(), &quotes[c], &q);
                quoted[c] = q;
                len += csv::utf8_length(f.str.size(), quotes[c], q);
            } else if (types[c] >= 10) {
                fmt::Dec d;
                fmt::dec_from_value(d, types[c], f.bits);
                len += (unsigned long long)fmt::fmt_length(d);
            } else {
                len += (unsigned long long)fmt::fmt_length_int(types[c], f.bits);
            }
        }
        if (csv::empty_record(ncols, len)) len = 2;
        len += (unsigned long long)ncols;
        // ---- write (k_csv_write) into exactly `len` bytes
        unsigned char* block = (unsigned char*)malloc((size_t)len);
        unsigned char* q = block;
        for (int c = 0; c < ncols; ++c) {
            if (c) *q++ = ',';
            const Field& f = row[c];
            if (!f.valid) continue;
            if (types[c] == 12) {
                q += csv::copy_field(q, f.str.data(), f.str.size(), quoted[c] != 0);
            } else {
                fmt::Dec d;
                fmt::dec_from_value(d, types[c], f.bits);
                const int n = fmt::fmt_length(d);
                for (int j = 0; j < n; ++j) q[j] = fmt::fmt_byte(d, j);
                q += n;
            }
        }
        if (csv::empty_record(ncols, (unsigned long long)(q - block))) {
            *q++ = '"';
            *q++ = '"';
        }
        *q++ = '\n';
        bad_len += (unsigned long long)(q - block) != len;
        fwrite(block, 1, (size_t)len, out);
        free(block);
        total += len;
    }
    fclose(in);
    fclose(out);
    printf("records %lld bytes %llu length mismatches %ld mask mismatches %ld\n", nrows, total, bad_len, bad_mask);
    if (bad_len || bad_mask) return 1;
    printf("clean\n");
    return 0;
}
