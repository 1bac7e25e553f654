// dfmi_sort_batches: ORDER BY / LIMIT over device batches (DFMI_FLAG_EXT_SORT;
// kernels in sort.hip, protocol in sort.h). The reference plans Sort and Limit
// (sqlplanner.rs:119-163) and its executor stops at context.rs:161; the order
// is DESIGN.md §2's key order, stable, a null greater than every value, DESC
// the whole comparison reversed.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "agg_state.h"
#include "sort.h"
#include "sort_key.h"

namespace dfmi {
namespace srt {
namespace {

// Select switch point (DESIGN.md §6 "ORDER BY"): the radix select runs when
// the input has at least kSelectMinRows rows and LIMIT keeps at most one row
// in kSelectRatio.
constexpr int64_t kSelectMinRows = 1 << 16;
constexpr int64_t kSelectRatio = 8;

enum Phase { kPhaseSelect = 0, kPhaseWord, kPhaseRadix, kPhaseGather, kPhases };

struct Scratch {
    HostBuf<uint8_t> htable;  // the batch table, pinned (one H2D copy per call)
    DevBuf table;
    DevBuf words[2], perm[2], tmp;
    DevBuf state, hist, counts;  // radix select
    DevBuf lens;                 // Utf8 gather
    DevBuf sums;                 // per column: null count; Utf8 bytes; [2 * ncols]: a key's longest string
    HostBuf<unsigned long long> hsums;
    // DFMI_DIAG=1 DFMI_SORT_PROFILE=1: device time of the last call's phases (dfmi_internal_sort_phases)
    std::vector<hipEvent_t> events;
    double phase_ms[kPhases] = {0, 0, 0, 0};
    // the last call (dfmi_internal_sort_select): did the top-k prefilter run, and the rows the radix passes got
    bool select_ran = false;
    unsigned long long select_rows = 0;
    ~Scratch() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
};

// HIP events between the launches of one call, read after its last synchronisation.
struct PhaseClock {
    Scratch& S;
    bool on;
    size_t used = 0;
    std::vector<int> phase;  // phase of the interval that ends at event i + 1
    PhaseClock(Scratch& s, bool enable) : S(s), on(enable) {}
    void mark(int ph, hipStream_t st) {  // the work since the last mark was phase `ph` (-1: the start)
        if (!on) return;
        if (used == S.events.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            S.events.push_back(e);
        }
        HIP_TRY(hipEventRecord(S.events[used++], st));
        if (ph >= 0) phase.push_back(ph);
    }
    void finish() {  // (the stream is idle)
        if (!on) return;
        for (double& m : S.phase_ms) m = 0;
        for (size_t i = 0; i + 1 < used; ++i) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, S.events[i], S.events[i + 1]));
            S.phase_ms[phase[i]] += ms;
        }
    }
};

Scratch& scratch(dfmi_context* ctx) {
    if (!ctx->sort_scratch) ctx->sort_scratch = new Scratch();
    return *(Scratch*)ctx->sort_scratch;
}

int bit_length(unsigned long long v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// DFMI_DIAG=1 DFMI_SORT_SELECT=0 / 1 forces the top-k prefilter off / on (read per call).
int forced_select() {
    if (!getenv("DFMI_DIAG")) return -1;
    const char* e = getenv("DFMI_SORT_SELECT");
    return e ? (atoi(e) != 0) : -1;
}

bool profiling() { return getenv("DFMI_DIAG") && getenv("DFMI_SORT_PROFILE"); }

void bad(const char* m) { throw Fail{DFMI_ERR_INVALID_ARGUMENT, m}; }

}  // namespace

int32_t sort_batches(dfmi_context* ctx, const dfmi_batch* in, int32_t nb, const int32_t* key_columns,
                     const int32_t* key_asc, int32_t nkeys, int64_t limit, dfmi_out_column* outs, uint32_t flags) {
    if (!ctx || !in || !outs) bad("dfmi_sort_batches: NULL argument");
    if (!(flags & DFMI_FLAG_EXT_SORT)) bad("dfmi_sort_batches needs DFMI_FLAG_EXT_SORT");
    if (nb < 1) bad("dfmi_sort_batches: no batch");
    if (nkeys < 0 || (nkeys > 0 && (!key_columns || !key_asc))) bad("dfmi_sort_batches: NULL key list");
    if (nkeys > kMaxKeys) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: more than 8 ORDER BY expressions"};
    const int ncols = in[0].num_columns;
    if (ncols < 1 || !in[0].columns) bad("dfmi_sort_batches: a batch without columns");
    for (int k = 0; k < nkeys; ++k)
        if (key_columns[k] < 0 || key_columns[k] >= ncols) bad("dfmi_sort_batches: key column out of range");

    // the batches: one schema, buffers present
    std::vector<int> type(ncols), has_nulls(ncols, 0);
    for (int j = 0; j < ncols; ++j) {
        type[j] = in[0].columns[j].type;
        if (type[j] < DFMI_TYPE_BOOLEAN || type[j] > DFMI_TYPE_UTF8) bad("dfmi_sort_batches: column type");
    }
    int64_t total = 0;
    for (int b = 0; b < nb; ++b) {
        if (in[b].num_columns != ncols || !in[b].columns || in[b].num_rows < 0) bad("dfmi_sort_batches: batch shape");
        for (int j = 0; j < ncols; ++j) {
            const dfmi_column& c = in[b].columns[j];
            if (c.type != type[j]) bad("dfmi_sort_batches: the batches differ in a column's type");
            if (c.length != in[b].num_rows || c.offset < 0) bad("dfmi_sort_batches: column length");
            if (in[b].num_rows > 0 && (!c.values || (type[j] == DFMI_TYPE_UTF8 && !c.offsets)))
                bad("dfmi_sort_batches: NULL column buffer");
            if (c.validity && c.null_count > 0 && in[b].num_rows > 0) has_nulls[j] = 1;
        }
        total += in[b].num_rows;
        if (total >= (int64_t(1) << 31))
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: 2^31 or more rows to sort"};
    }
    const unsigned n = (unsigned)total;
    for (int j = 0; j < ncols; ++j) {
        const dfmi_out_column& o = outs[j];
        if (!n) continue;
        if (type[j] == DFMI_TYPE_UTF8 ? (!o.offsets || !o.data) : !o.values) bad("dfmi_sort_batches: NULL output buffer");
        if (has_nulls[j] && !o.validity) bad("dfmi_sort_batches: NULL output validity");
    }

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Scratch& S = scratch(ctx);
    S.select_ran = false;
    S.select_rows = 0;

    auto finish_empty = [&]() {
        for (int j = 0; j < ncols; ++j) {
            dfmi_out_column& o = outs[j];
            o.type = type[j];
            o.passthrough_column = -1;
            o.length = o.null_count = o.data_length = 0;
            if (type[j] == DFMI_TYPE_UTF8 && o.offsets) HIP_TRY(hipMemsetAsync(o.offsets, 0, sizeof(int32_t), st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        return (int32_t)DFMI_OK;
    };
    if (!n || limit == 0) return finish_empty();

    // ---- the batch table: row prefix, then per column one ColPtr per batch
    const size_t prefix_bytes = (((size_t)nb + 1) * sizeof(unsigned) + 15) & ~(size_t)15;
    const size_t table_bytes = prefix_bytes + (size_t)ncols * nb * sizeof(ColPtr);
    S.htable.resize(table_bytes);
    {
        unsigned* prefix = (unsigned*)S.htable.data();
        ColPtr* cp = (ColPtr*)(S.htable.data() + prefix_bytes);
        unsigned at = 0;
        for (int b = 0; b < nb; ++b) {
            prefix[b] = at;
            at += (unsigned)in[b].num_rows;
            for (int j = 0; j < ncols; ++j) {
                const dfmi_column& c = in[b].columns[j];
                cp[(size_t)j * nb + b] = ColPtr{c.values, c.null_count > 0 ? c.validity : nullptr, c.offsets, c.offset};
            }
        }
        prefix[nb] = at;
    }
    S.table.reserve(table_bytes);
    HIP_TRY(hipMemcpyAsync(S.table.p, S.htable.data(), table_bytes, hipMemcpyHostToDevice, st));
    const Rows rows{S.table.as<unsigned>(), nb, n};
    auto col_ptrs = [&](int j) { return (const ColPtr*)(S.table.as<uint8_t>() + prefix_bytes) + (size_t)j * nb; };

    // ---- scratch, sized before anything is enqueued on it (a growing buffer drops its contents)
    S.sums.reserve((size_t)(2 * ncols + 1) * sizeof(unsigned long long));
    S.hsums.resize((size_t)2 * ncols + 1);
    unsigned long long* dsum = S.sums.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(dsum, 0, (size_t)(2 * ncols + 1) * sizeof(unsigned long long), st));
    const unsigned tiles = (n + kSelectRows - 1) / kSelectRows;
    size_t tmp_bytes = 0;
    if (nkeys > 0) {
        for (int i = 0; i < 2; ++i) {
            S.words[i].reserve((size_t)n * sizeof(unsigned long long));
            S.perm[i].reserve((size_t)n * sizeof(unsigned));
        }
        size_t b = 0;
        HIP_TRY(radix_pass(nullptr, &b, nullptr, nullptr, nullptr, nullptr, n, 64, st));
        tmp_bytes = std::max(tmp_bytes, b);
        S.state.reserve(sizeof(SelectState));
        S.hist.reserve(kSelectBins * sizeof(unsigned));
        S.counts.reserve((size_t)2 * (tiles + 1) * sizeof(unsigned));
        HIP_TRY(launch_select(nullptr, n, 64, 1, nullptr, nullptr, S.counts.as<unsigned>(), nullptr, &b, nullptr, st));
        tmp_bytes = std::max(tmp_bytes, b);
    }
    bool any_utf8 = false;
    for (int j = 0; j < ncols; ++j) any_utf8 |= type[j] == DFMI_TYPE_UTF8;
    if (any_utf8) {
        S.lens.reserve(((size_t)n + 1) * sizeof(unsigned));
        size_t b = 0;
        HIP_TRY(scan_offsets(nullptr, &b, nullptr, nullptr, n, st));
        tmp_bytes = std::max(tmp_bytes, b);
    }
    S.tmp.reserve(tmp_bytes);

    unsigned long long* words[2] = {S.words[0].as<unsigned long long>(), S.words[1].as<unsigned long long>()};
    unsigned* perm[2] = {S.perm[0].as<unsigned>(), S.perm[1].as<unsigned>()};
    int cur = 0;             // perm[cur] is the permutation so far ...
    bool have_perm = false;  // ... once there is one (else: the input order)
    unsigned ns = n;         // rows to sort

    auto key_word = [&](int k, int what, int chunk, bool null_above, unsigned count) {
        WordArgs a{};
        a.rows = rows;
        a.col = col_ptrs(key_columns[k]);
        a.type = type[key_columns[k]];
        a.what = what;
        a.chunk = chunk;
        a.asc = key_asc[k] != 0;
        a.has_nulls = has_nulls[key_columns[k]];
        a.null_above = null_above;
        a.perm = have_perm ? perm[cur] : nullptr;
        a.perm_out = have_perm ? nullptr : perm[cur];
        a.n = count;
        a.words = words[0];
        HIP_TRY(launch_word(a, st));
    };

    PhaseClock clock(S, profiling());
    clock.mark(-1, st);

    // ---- top-k prefilter: the rows whose leading word is <= the limit-th smallest, in input order
    const int forced = forced_select();
    const bool select = nkeys > 0 && limit > 0 && limit < (int64_t)n &&
                        (forced >= 0 ? forced == 1 : ((int64_t)n >= kSelectMinRows && limit * kSelectRatio <= (int64_t)n));
    if (select) {
        const int t = type[key_columns[0]];
        const bool above = t != DFMI_TYPE_UTF8 && sort_value_bits(t) <= 32 && has_nulls[key_columns[0]];
        const int bits = t == DFMI_TYPE_UTF8 ? 64 : sort_value_bits(t) + (above ? 1 : 0);
        key_word(0, kWordSelect, 0, above, n);
        size_t b = tmp_bytes;
        HIP_TRY(launch_select(words[0], n, bits, (unsigned long long)limit, S.state.as<SelectState>(),
                               S.hist.as<unsigned>(), S.counts.as<unsigned>(), S.tmp.p, &b, perm[cur], st));
        HIP_TRY(hipMemcpyAsync(S.hsums.data(), &S.state.as<SelectState>()->total, sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned long long cand = S.hsums[0];
        if (cand < (unsigned long long)limit || cand > n)
            throw Fail{DFMI_ERR_DEVICE, "dfmi_sort_batches: the radix select lost rows"};
        ns = (unsigned)cand;
        have_perm = true;
        clock.mark(kPhaseSelect, st);
    }
    S.select_ran = select;
    S.select_rows = ns;

    // ---- the permutation: LSD passes, last key first
    auto pass = [&](int k, int what, int chunk, bool null_above, int end_bit) {
        key_word(k, what, chunk, null_above, ns);
        clock.mark(kPhaseWord, st);
        size_t b = tmp_bytes;
        HIP_TRY(radix_pass(S.tmp.p, &b, words[0], words[1], perm[cur], perm[cur ^ 1], ns, end_bit, st));
        clock.mark(kPhaseRadix, st);
        cur ^= 1;
        have_perm = true;
    };
    for (int k = nkeys - 1; k >= 0 && ns > 1; --k) {
        const int j = key_columns[k], t = type[j];
        if (t == DFMI_TYPE_UTF8) {
            unsigned long long* dmax = dsum + 2 * ncols;
            HIP_TRY(hipMemsetAsync(dmax, 0, sizeof *dmax, st));
            Utf8Args u{};
            u.rows = rows;
            u.col = col_ptrs(j);
            u.total = dmax;
            HIP_TRY(launch_utf8_max(u, st));
            clock.mark(kPhaseWord, st);
            HIP_TRY(hipMemcpyAsync(S.hsums.data() + 2 * ncols, dmax, sizeof *dmax, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const unsigned long long maxlen = S.hsums[2 * ncols];
            pass(k, kWordLength, 0, false, std::max(1, bit_length(maxlen)));
            for (int c = (int)((maxlen + 7) / 8) - 1; c >= 0; --c) pass(k, kWordChunk, c, false, 64);
            if (has_nulls[j]) pass(k, kWordNull, 0, false, 1);
        } else {
            const int vb = sort_value_bits(t);
            const bool above = vb <= 32 && has_nulls[j];
            pass(k, kWordValue, 0, above, vb + (above ? 1 : 0));
            if (has_nulls[j] && !above) pass(k, kWordNull, 0, false, 1);
        }
    }

    // ---- gather every column by the permutation
    const unsigned m = limit < 0 ? ns : (unsigned)std::min<int64_t>(limit, ns);
    const unsigned* order = have_perm ? perm[cur] : nullptr;
    for (int j = 0; j < ncols; ++j) {
        dfmi_out_column& o = outs[j];
        if (has_nulls[j]) {
            BitsArgs v{rows, col_ptrs(j), order, m, 1, (unsigned long long*)o.validity, dsum + j};
            HIP_TRY(launch_gather_bits(v, st));
        }
        if (type[j] == DFMI_TYPE_BOOLEAN) {
            BitsArgs v{rows, col_ptrs(j), order, m, 0, (unsigned long long*)o.values, nullptr};
            HIP_TRY(launch_gather_bits(v, st));
        } else if (type[j] == DFMI_TYPE_UTF8) {
            Utf8Args u{};
            u.rows = rows;
            u.col = col_ptrs(j);
            u.perm = order;
            u.m = m;
            u.lens = S.lens.as<unsigned>();
            u.total = dsum + ncols + j;
            HIP_TRY(launch_utf8_len(u, st));
            HIP_TRY(hipMemcpyAsync(S.hsums.data() + ncols + j, u.total, sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const unsigned long long bytes = S.hsums[ncols + j];
            if (bytes >= (1ull << 31))
                throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: 2^31 or more bytes in a Utf8 column to sort"};
            if ((int64_t)bytes > o.data_capacity)
                throw Fail{DFMI_ERR_CAPACITY, "dfmi_sort_batches: Utf8 data_capacity too small"};
            size_t b = tmp_bytes;
            HIP_TRY(scan_offsets(S.tmp.p, &b, u.lens, o.offsets, m, st));
            u.out_offsets = o.offsets;
            u.out_data = o.data;
            HIP_TRY(launch_utf8_copy(u, st));
        } else {
            GatherArgs g{rows, col_ptrs(j), order, m, o.values};
            HIP_TRY(launch_gather(g, type_width(type[j]), st));
        }
    }
    clock.mark(kPhaseGather, st);
    HIP_TRY(hipMemcpyAsync(S.hsums.data(), dsum, (size_t)ncols * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    clock.finish();
    for (int j = 0; j < ncols; ++j) {
        dfmi_out_column& o = outs[j];
        o.type = type[j];
        o.passthrough_column = -1;
        o.length = m;
        o.null_count = has_nulls[j] ? (int64_t)S.hsums[j] : 0;
        o.data_length = type[j] == DFMI_TYPE_UTF8 ? (int64_t)S.hsums[ncols + j] : 0;
    }
    return DFMI_OK;
}

}  // namespace srt

void sort_scratch_release(dfmi_context* c) {
    delete (srt::Scratch*)c->sort_scratch;
    c->sort_scratch = nullptr;
}

}  // namespace dfmi

// Diagnostics (DFMI_DIAG=1 DFMI_SORT_PROFILE=1): device milliseconds of the last dfmi_sort_batches on ctx --
// the top-k select, the key words, the radix passes, the gather.
extern "C" int32_t dfmi_internal_sort_phases(const dfmi_context* ctx, double* ms) {
    if (!ctx || !ctx->sort_scratch || !ms) return DFMI_ERR_INVALID_ARGUMENT;
    const dfmi::srt::Scratch& S = *(const dfmi::srt::Scratch*)ctx->sort_scratch;
    for (int i = 0; i < dfmi::srt::kPhases; ++i) ms[i] = S.phase_ms[i];
    return DFMI_OK;
}

// Diagnostics: which path the last dfmi_sort_batches on ctx took -- out[0] is 1 if the top-k prefilter ran,
// out[1] the number of rows handed to the radix passes (every input row without the prefilter).
extern "C" int32_t dfmi_internal_sort_select(const dfmi_context* ctx, uint64_t out[2]) {
    if (!ctx || !ctx->sort_scratch || !out) return DFMI_ERR_INVALID_ARGUMENT;
    const dfmi::srt::Scratch& S = *(const dfmi::srt::Scratch*)ctx->sort_scratch;
    out[0] = S.select_ran ? 1 : 0;
    out[1] = S.select_rows;
    return DFMI_OK;
}

extern "C" int32_t dfmi_sort_batches(dfmi_context* ctx, const dfmi_batch* inputs, int32_t num_batches,
                                     const int32_t* key_columns, const int32_t* key_asc, int32_t num_keys,
                                     int64_t limit, dfmi_out_column* outputs, uint32_t flags, dfmi_error* err) {
    return dfmi::xi::guarded(err, [&]() -> int32_t {
        return dfmi::srt::sort_batches(ctx, inputs, num_batches, key_columns, key_asc, num_keys, limit, outputs, flags);
    });
}
