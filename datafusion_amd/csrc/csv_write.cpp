// dfmi_csv_header and dfmi_csv_encode_batches: result batches as CSV
// (DFMI_FLAG_EXT_CSV_WRITE; kernels in csv_write.hip, protocol in csv_write.h,
// the field rules in csv_field.h, the numbers' bytes in format_core.h). One
// call encodes all batches of a coalesced pull into one byte stream: quote
// scan (Utf8 columns only), measure, scan, write -- one launch of each.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "agg_state.h"
#include "csv_field.h"
#include "csv_write.h"
#include "slice.h"

namespace dfmi {
namespace csvk {
namespace {

// The per-row scratch -- `lens` and `sums`, 8 bytes a padded row together, a quote word per row and Utf8
// column, and the scan's `tmp` -- only grows and stays with the context until dfmi_context_destroy, as the
// format scratch does (include/dfmi.h says so).
struct Scratch {
    HostBuf<uint8_t> htable;  // the column, batch and Utf8-column tables, pinned (one H2D copy per call)
    DevBuf table, totals;
    DevBuf lens, sums, tmp, quote;
    HostBuf<unsigned long long> htotals;
    // DFMI_DIAG=1: the last call's device time per phase -- quote scan, measure, scan, write (the probe's figures)
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float phase_ms[4] = {0, 0, 0, 0};
    ~Scratch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

Scratch& scratch(dfmi_context* ctx) {
    if (!ctx->csv_scratch) ctx->csv_scratch = new Scratch();
    return *(Scratch*)ctx->csv_scratch;
}

// DFMI_DIAG=1 DFMI_CSV_GRID=n: at most n workgroups per launch (read per call).
unsigned grid_cap() {
    if (!getenv("DFMI_DIAG")) return kMaxGrid;
    const char* e = getenv("DFMI_CSV_GRID");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? (unsigned)std::min<int>(v, (int)kMaxGrid) : kMaxGrid;
}

void bad(const char* m) { throw Fail{DFMI_ERR_INVALID_ARGUMENT, m}; }

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

int32_t csv_header(const dfmi_schema* schema, uint8_t* out, int64_t capacity, int64_t* length) {
    if (!schema || !length) bad("dfmi_csv_header: NULL argument");
    if (schema->num_fields < 1 || !schema->fields) bad("dfmi_csv_header: a schema without fields");
    if (capacity < 0 || (capacity > 0 && !out)) bad("dfmi_csv_header: NULL buffer");
    const int n = schema->num_fields;
    unsigned long long need = 0;
    std::vector<unsigned long long> quotes((size_t)n);
    std::vector<char> quoted((size_t)n);
    for (int i = 0; i < n; ++i) {
        const char* s = schema->fields[i].name;
        if (!s) bad("dfmi_csv_header: NULL field name");
        bool q = false;
        csv::scan_field((const unsigned char*)s, strlen(s), &quotes[i], &q);
        quoted[i] = q;
        need += csv::utf8_length(strlen(s), quotes[i], q);
    }
    if (csv::empty_record(n, need)) need = 2;
    need += (unsigned long long)n;
    *length = (int64_t)need;
    if (!out) return DFMI_OK;  // measure only
    if ((unsigned long long)capacity < need) throw Fail{DFMI_ERR_CAPACITY, "dfmi_csv_header: capacity too small"};
    uint8_t* p = out;
    for (int i = 0; i < n; ++i) {
        if (i) *p++ = ',';
        const char* s = schema->fields[i].name;
        p += csv::copy_field(p, (const unsigned char*)s, strlen(s), quoted[i] != 0);
    }
    if (csv::empty_record(n, (unsigned long long)(p - out))) {
        *p++ = '"';
        *p++ = '"';
    }
    *p = '\n';
    return DFMI_OK;
}

int32_t csv_encode_batches(dfmi_context* ctx, const dfmi_batch* inputs, int32_t nb, uint8_t* data, int64_t capacity,
                           int64_t* data_length, int64_t* batch_ends, uint32_t flags) {
    if (!(flags & DFMI_FLAG_EXT_CSV_WRITE))
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "dfmi_csv_encode_batches needs DFMI_FLAG_EXT_CSV_WRITE"};
    if (!ctx || !data_length || nb < 0) bad("dfmi_csv_encode_batches: NULL argument");
    *data_length = 0;
    if (nb == 0) return DFMI_OK;
    if (!inputs) bad("dfmi_csv_encode_batches: NULL argument");
    if (data && capacity < 0) bad("dfmi_csv_encode_batches: negative data_capacity");
    const int ncols = inputs[0].num_columns;
    if (ncols > kMaxColumns)
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: more than 256 columns to encode as CSV"};
    if (ncols < 1) bad("dfmi_csv_encode_batches: a batch without columns");
    int64_t total = 0;
    for (int32_t b = 0; b < nb; ++b) {
        const dfmi_batch& in = inputs[b];
        if (in.num_columns != ncols) bad("dfmi_csv_encode_batches: batches of different column counts");
        if (!in.columns) bad("dfmi_csv_encode_batches: NULL argument");
        if (in.num_rows < 0) bad("dfmi_csv_encode_batches: batch length");
        for (int i = 0; i < ncols; ++i) {
            const dfmi_column& c = in.columns[i];
            if (c.type < DFMI_TYPE_BOOLEAN || c.type > DFMI_TYPE_UTF8) bad("dfmi_csv_encode_batches: column type");
            if (c.type != inputs[0].columns[i].type) bad("dfmi_csv_encode_batches: batches of different column types");
            if (c.length != in.num_rows || c.offset < 0) bad("dfmi_csv_encode_batches: column length");
            if (in.num_rows > 0 && !c.values) bad("dfmi_csv_encode_batches: NULL column buffer");
            if (in.num_rows > 0 && c.type == DFMI_TYPE_UTF8 && !c.offsets) bad("dfmi_csv_encode_batches: NULL column buffer");
        }
        total += in.num_rows;
        if (total >= (int64_t(1) << 31))
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: 2^31 or more rows to encode as CSV"};
    }

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Scratch& S = scratch(ctx);
    Unsliced U;
    const dfmi_batch* bs = inputs;
    if (any_offset(bs, nb)) bs = unslice(bs, nb, U, true, st);

    std::vector<int> utf8;
    for (int i = 0; i < ncols; ++i)
        if (inputs[0].columns[i].type == DFMI_TYPE_UTF8) utf8.push_back(i);
    const int nutf8 = (int)utf8.size();

    // ---- scratch, sized before anything is enqueued on it (a growing buffer drops its contents)
    unsigned tiles = 0;
    for (int32_t b = 0; b < nb; ++b) tiles += ((unsigned)bs[b].num_rows + kTileRows - 1) / kTileRows;  // (< 2^31 rows)
    const size_t slots = (size_t)tiles * kTileRows + 1;
    const size_t cols_bytes = (size_t)nb * ncols * sizeof(Col), batches_bytes = align8((size_t)nb * sizeof(Batch));
    const size_t table_bytes = cols_bytes + batches_bytes + align8((size_t)nutf8 * sizeof(int));
    const size_t quote_words = (size_t)nutf8 * (size_t)total;
    S.htable.resize(table_bytes);
    S.table.reserve(table_bytes);
    S.lens.reserve(slots * sizeof(unsigned));
    S.sums.reserve(slots * sizeof(unsigned));
    S.totals.reserve((size_t)nb * sizeof(unsigned long long));
    S.htotals.resize((size_t)nb);
    if (quote_words) S.quote.reserve(quote_words * sizeof(unsigned));

    // ---- the tables
    Col* hc = (Col*)S.htable.data();
    Batch* hb = (Batch*)(S.htable.data() + cols_bytes);
    int* hu = (int*)(S.htable.data() + cols_bytes + batches_bytes);
    unsigned t0 = 0;
    size_t q0 = 0;
    for (int32_t b = 0; b < nb; ++b) {
        const unsigned n = (unsigned)bs[b].num_rows;
        hb[b].n = n;
        hb[b].tile0 = t0;
        t0 += (n + kTileRows - 1) / kTileRows;
        for (int i = 0; i < ncols; ++i) {
            const dfmi_column& c = bs[b].columns[i];
            Col& k = hc[(size_t)b * ncols + i];
            k.values = c.values;
            k.validity = n > 0 && c.validity && c.null_count > 0 ? c.validity : nullptr;
            k.offsets = c.offsets;
            k.quote = nullptr;
            k.type = c.type;
            k.pad = 0;
            if (c.type == DFMI_TYPE_UTF8) {
                k.quote = S.quote.as<unsigned>() + q0;
                q0 += n;
            }
        }
    }
    for (int i = 0; i < nutf8; ++i) hu[i] = utf8[i];

    Args A{};
    A.cols = S.table.as<Col>();
    A.batches = (const Batch*)(S.table.as<uint8_t>() + cols_bytes);
    A.utf8_cols = (const int*)(S.table.as<uint8_t>() + cols_bytes + batches_bytes);
    A.nbatches = nb;
    A.ncols = ncols;
    A.nutf8 = nutf8;
    A.tiles = tiles;
    A.lens = S.lens.as<unsigned>();
    A.sums = S.sums.as<unsigned>();
    A.totals = S.totals.as<unsigned long long>();
    A.data = data;
    size_t tmp_bytes = 0;
    HIP_TRY(scan_lengths(nullptr, &tmp_bytes, A, st));
    S.tmp.reserve(tmp_bytes);

    HIP_TRY(hipMemcpyAsync(S.table.p, S.htable.data(), table_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(A.totals, 0, (size_t)nb * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(A.lens + (slots - 1), 0, sizeof(unsigned), st));
    if (quote_words) HIP_TRY(hipMemsetAsync(S.quote.p, 0, quote_words * sizeof(unsigned), st));
    const unsigned grid = std::max(1u, std::min(tiles, grid_cap()));
    const bool diag = getenv("DFMI_DIAG") != nullptr;
    auto stamp = [&](int k) {
        if (!diag) return;
        if (!S.ev[k]) HIP_TRY(hipEventCreate(&S.ev[k]));
        HIP_TRY(hipEventRecord(S.ev[k], st));
    };
    auto phase = [&](int k, int e0) {  // (after a synchronise)
        if (diag) HIP_TRY(hipEventElapsedTime(&S.phase_ms[k], S.ev[e0], S.ev[e0 + 1]));
    };
    for (float& v : S.phase_ms) v = 0;
    stamp(0);
    HIP_TRY(launch_quote_scan(A, grid, st));
    stamp(1);
    HIP_TRY(launch_measure(A, grid, st));
    stamp(2);
    HIP_TRY(hipMemcpyAsync(S.htotals.data(), A.totals, (size_t)nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    phase(0, 0);
    phase(1, 1);

    // ---- the bytes the call needs: reported whatever follows
    unsigned long long need = 0;
    for (int32_t b = 0; b < nb; ++b) {
        need += S.htotals[b];  // (fewer than 2^31 rows of fewer than 2^40 bytes each: no wrap)
        if (batch_ends) batch_ends[b] = (int64_t)need;
    }
    *data_length = (int64_t)need;
    if (need >= (1ull << 31))
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: CSV output of 2^31 or more bytes"};
    if (!data) return DFMI_OK;  // measure only
    if ((int64_t)need > capacity) throw Fail{DFMI_ERR_CAPACITY, "dfmi_csv_encode_batches: data_capacity too small"};

    stamp(3);
    HIP_TRY(scan_lengths(S.tmp.p, &tmp_bytes, A, st));
    stamp(4);
    HIP_TRY(launch_write(A, grid, st));
    stamp(5);
    HIP_TRY(hipStreamSynchronize(st));
    phase(2, 3);
    phase(3, 4);
    return DFMI_OK;
}

}  // namespace csvk

void csv_scratch_release(dfmi_context* c) {
    delete (csvk::Scratch*)c->csv_scratch;
    c->csv_scratch = nullptr;
}

}  // namespace dfmi

// Diagnostics (DFMI_DIAG=1): the device time in ms of the last dfmi_csv_encode_batches on ctx per phase --
// out[0] quote scan, out[1] measure, out[2] scan, out[3] write (0 for a phase that did not run).
extern "C" int32_t dfmi_internal_csv_phases(const dfmi_context* ctx, double out[4]) {
    if (!ctx || !ctx->csv_scratch || !out) return DFMI_ERR_INVALID_ARGUMENT;
    const dfmi::csvk::Scratch& S = *(const dfmi::csvk::Scratch*)ctx->csv_scratch;
    for (int k = 0; k < 4; ++k) out[k] = S.phase_ms[k];
    return DFMI_OK;
}

extern "C" int32_t dfmi_csv_header(const dfmi_schema* schema, uint8_t* out, int64_t capacity, int64_t* length,
                                   dfmi_error* err) {
    return dfmi::xi::guarded(err, [&]() -> int32_t { return dfmi::csvk::csv_header(schema, out, capacity, length); });
}

extern "C" int32_t dfmi_csv_encode_batches(dfmi_context* ctx, const dfmi_batch* inputs, int32_t num_batches,
                                           uint8_t* data, int64_t data_capacity, int64_t* data_length,
                                           int64_t* batch_ends, uint32_t flags, dfmi_error* err) {
    return dfmi::xi::guarded(err, [&]() -> int32_t {
        return dfmi::csvk::csv_encode_batches(ctx, inputs, num_batches, data, data_capacity, data_length, batch_ends,
                                              flags);
    });
}
