// Aggregate extension: the state behind dfmi_agg_state, the buffers it owns,
// and what the device hash table's driver (agg_hash.cpp) offers the entry
// points (aggregate.cpp).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <unordered_map>
#include <vector>

#include "agg_host.h"
#include "exec_internal.h"
#include "groupby.h"
#include "str_extreme.h"

namespace dfmi {
namespace agg {

// The device hash table of a grouped state (groupby.h; kernels in groupby.hip).
struct HashDev {
    // The scratch buffers, one slot per use: no two uses that are live at the
    // same time share one.
    enum Slot {
        EvalOut = 0,  // the evaluation pass: up to three per output column (values or offsets + bytes, validity)
        DrainNull = EvalOut + 3 * (dfmi::gb::kMaxKeys + dfmi::gb::kMaxAggs),  // read_table / finish_device: the
        DrainKeyWords, DrainKeyLens,                                          // compacted keys,
        DrainRounded,                                                         // the records k_group_round finished
        // accumulate_bucketed: group id per row; per (bucket, block) counts, then starts; bucket totals; the batch
        // partitioned by bucket: group ids, NULL masks, payload words
        BucketRowGroup, BucketHist, BucketTotals, BucketPartGroup, BucketPartNull, BucketPartValues,
        // finish_device: the caller's arrays on the device; the radix sort's double buffers and scratch
        EmitKeys, EmitValues, EmitSortKeys, EmitSortKeys2, EmitSortVals, EmitSortVals2, EmitNullAt, EmitTemp,
        // a coalesced call: the evaluation pass's per-batch segments packed dense, two per output column
        // (values, validity); the pack kernel's source table, jobs and prefix
        PackOut, PackTable = PackOut + 2 * (dfmi::gb::kMaxKeys + dfmi::gb::kMaxAggs),
        // accumulate_hashed: the argument of a Boolean MIN / MAX as UInt8 0 / 1, one per aggregate
        BoolArg, kSlots = BoolArg + dfmi::gb::kMaxAggs
    };
    DevBuf ctl, slot;                 // the table's storage; `t` views it
    dfmi::gb::Table t{};
    uint64_t cap = 0;                 // slots
    DevBuf hdr;                       // dfmi::gb::Hdr: device counters
    HostBuf<dfmi::gb::Hdr> hh;        // pinned host copy
    DevBuf arena;                     // Utf8 key bytes
    uint64_t arena_cap = 0;
    DevBuf acc;                       // [acc_cap][words] group records
    uint64_t acc_cap = 0;
    DevBuf pattern;                   // one zero-state record (device)
    std::vector<uint64_t> hpattern;
    int words = 0;
    std::vector<int> off, foff;       // per aggregate: record offset; float SUMs: digit offsets
    DevBuf sidx, coll;
    int64_t rows_cap = 0;             // sidx / coll capacity
    uint32_t epoch = 0;
    uint64_t ngroups = 0;             // groups the device holds
    uint64_t rows_since_norm = 0;     // rows added since the digits were last carry-normalised
    DevBuf bufs[kSlots];              // scratch (the fused pass's output columns, drains, buckets, emission)

    dfmi::gb::Hdr* dhdr() const { return hdr.as<dfmi::gb::Hdr>(); }
    unsigned long long* records() const { return acc.as<unsigned long long>(); }
};

// The device hash table's groups as flat host arrays by group id (read_table;
// for a finish, `rounded`: the records finished on the device and the table
// left as it is):
// keys (null bits, words: the value bits or the Utf8 arena offset, lengths),
// the records, the Utf8 arena, and `order` -- the group ids in key order.
struct FlatGroups {
    bool rounded = false;  // acc: the device finish's compact records (groupby.h RoundArgs), the table kept
    uint64_t ng = 0;
    size_t nk = 0;
    int words = 0;
    std::vector<int> off;
    std::vector<uint32_t> order;
    HostBuf<unsigned> knull, klen;
    HostBuf<uint64_t> kw, acc;
    HostBuf<uint8_t> arena;
    // a state with Utf8 MIN / MAX aggregates: per extreme (StrExt::x order) the groups' persisted winners, and their arena
    std::vector<std::vector<dfmi::sx::Ent>> sx_ent;
    std::vector<uint8_t> sx_arena;
};

// The Utf8 MIN / MAX aggregates of a state (str_extreme.h): per extreme the
// side arrays over the dense group ids (one group when ungrouped), the
// string arena they share, and the ungrouped evaluation pass's buffers.
struct StrExt {
    struct One {
        int agg = 0;  // index among the state's aggregates
        bool is_min = false;
        DevBuf pref, best, ent;
    };
    std::vector<One> x;
    uint64_t gcap = 0;  // groups the side arrays hold (initialised)
    DevBuf arena, hdr;
    uint64_t arena_cap = 0;
    uint64_t arena_end = 0;  // the device counters after the last batch: bytes reserved,
    uint64_t live = 0;       // bytes of the persisted winners
    std::vector<DevBuf> eval;  // ungrouped: the evaluated argument columns (offsets, bytes, validity each)
    std::vector<dfmi::aggh::StrVal> one;  // ungrouped: the last finish's values, by aggregate
    bool finished = false;                // a finish has produced values (dfmi_agg_state_value_bytes)
};

}  // namespace agg
}  // namespace dfmi

struct dfmi_agg_state {
    int device = 0;
    std::vector<const dfmi_aggregate*> aggs;
    dfmi::DevBuf acc;  // uint64 [kAggCopies][n][kAggWords]; grouped: [kAggCopies][gslots][n + 1][kAggWords]
    size_t acc_words = 0;
    bool failed = false;      // a batch raised an error: the query has failed
    dfmi_error failure{};
    std::vector<uint64_t> init;  // the zero state (MIN keys all ones)
    // GROUP BY extension (dfmi_agg_state_create_grouped / _multi)
    bool grouped = false;
    std::vector<dfmi_program> keys;  // the key expressions (copies: same uid, same kernels)
    dfmi_program key;           // keys[0] (the window kernel's key)
    int gslots = 0;             // window slots per accumulator copy: the key window + the null slot
    uint64_t win_base = 0;      // the window the device accumulators hold ...
    int win_width = -1;         // ... (-1: none yet)
    bool dirty = false;         // the device window accumulators hold rows
    dfmi::aggh::GroupMap groups;  // merged groups (window flushes, hash-table drains, host merges)
    // the host merge's per-row lookup: encoded key -> entry of `groups` (map
    // nodes do not move), cleared with it
    std::unordered_map<std::string, dfmi::aggh::GroupState*> index;
    std::shared_ptr<dfmi::aggh::GroupMap> shown;  // groups dfmi_shard_agg_finish_grouped merged (else `groups`)
    std::unique_ptr<dfmi::agg::HashDev> hd;       // device hash table (created on first use)
    std::unique_ptr<dfmi::agg::FlatGroups> flat;  // a finish's groups, not yet in `groups` (finish_flat)
    std::unique_ptr<dfmi::agg::FlatGroups> spare_flat;  // a used one, its pinned buffers kept for the next drain
    std::unique_ptr<dfmi::agg::StrExt> sx;  // Utf8 MIN / MAX aggregates (null: none)
    // integer keys: the per-batch key window comes from MIN / MAX of the key
    // over the batch's selected rows (a pre-pass through this same extension)
    dfmi_aggregate* mm[2] = {nullptr, nullptr};
    dfmi_agg_state* mm_state = nullptr;
    // dfmi_aggregate_host_batches: the call's packed input columns, pinned and on the device
    dfmi::HostBuf<uint8_t> stage_host;
    dfmi::DevBuf stage_dev;
};

namespace dfmi {
namespace agg {

// The diagnostic knobs of the aggregate path (DFMI_DIAG=1 and ...), read once
// per entry point -- per call, never cached: tests switch them within one
// process -- and nothing but DFMI_DIAG read when that is unset. A knob that
// carries a value is its text, null when unset.
struct AggDiag {
    bool group_host = false;      // DFMI_GROUP_HOST: every batch merged on the host (A/B of the hash table)
    bool host_finish = false;     // DFMI_GROUP_HOST_FINISH: no device rounding / emission
    bool finish_profile = false;  // DFMI_FINISH_PROFILE: timings on stderr
    const char* buckets = nullptr;          // DFMI_GROUP_BUCKETS=0 / 1
    const char* device_emit = nullptr;      // DFMI_GROUP_DEVICE_EMIT=0 / 1
    const char* hash_bits = nullptr;        // DFMI_GROUP_HASH_BITS
    const char* subtiles = nullptr;         // DFMI_AGG_SUBTILES
    const char* rows_per_thread = nullptr;  // DFMI_ROWS_PER_THREAD
    const char* proj_dense = nullptr;       // DFMI_PROJ_DENSE
    const char* group_norm_rows = nullptr;  // DFMI_GROUP_NORM_ROWS
    const char* group_grid = nullptr;       // DFMI_GROUP_GRID
};

// Rows a grouped state's exact-sum digits absorb between two carry
// normalisations (accumulate_hashed).
constexpr uint64_t kGroupNormRows = 1ull << 30;

inline AggDiag agg_diag() {
    AggDiag d;
    if (!getenv("DFMI_DIAG")) return d;
    d.group_host = getenv("DFMI_GROUP_HOST") != nullptr;
    d.host_finish = getenv("DFMI_GROUP_HOST_FINISH") != nullptr;
    d.finish_profile = getenv("DFMI_FINISH_PROFILE") != nullptr;
    d.buckets = getenv("DFMI_GROUP_BUCKETS");
    d.device_emit = getenv("DFMI_GROUP_DEVICE_EMIT");
    d.hash_bits = getenv("DFMI_GROUP_HASH_BITS");
    d.subtiles = getenv("DFMI_AGG_SUBTILES");
    d.rows_per_thread = getenv("DFMI_ROWS_PER_THREAD");
    d.proj_dense = getenv("DFMI_PROJ_DENSE");
    d.group_norm_rows = getenv("DFMI_GROUP_NORM_ROWS");
    d.group_grid = getenv("DFMI_GROUP_GRID");
    return d;
}

// DFMI_GROUP_NORM_ROWS (diagnostics): the normalisation threshold lowered to
// its value, clamped to [0, kGroupNormRows] -- the knob never raises it; 0: a
// carry pass before every batch that adds rows.
inline uint64_t group_norm_rows(const AggDiag& diag) {
    if (!diag.group_norm_rows) return kGroupNormRows;
    const long long v = atoll(diag.group_norm_rows);
    return v < 0 ? 0 : std::min<uint64_t>((uint64_t)v, kGroupNormRows);
}

// DFMI_GROUP_GRID (diagnostics): the workgroups of every launch of groupby.hip
// and str_extreme.hip lowered to at most its value (groupby.h "Diagnostic grid
// cap"; each launch clamps it to [1, its own cap] -- the knob never raises a
// grid). 0: unset, every launch's own grid.
inline int group_grid(const AggDiag& diag) {
    if (!diag.group_grid) return 0;
    const long long v = atoll(diag.group_grid);
    return v < 1 ? 1 : (int)std::min<long long>(v, 1 << 30);
}

// The sticky failure of a state: a batch has failed the query.
inline void check_not_failed(const dfmi_agg_state* st) {
    if (st->failed) throw Fail{st->failure.code, st->failure.message};
}

// ---- aggregate.cpp: one aggregate batch's plan; the key window's flush
// Static errors, slots and tile shape of one aggregate batch.
struct AggBuilt {
    xi::Err se;
    jit::Plan plan;
    jit::Launch X;
    int64_t n_tiles = 0;
};
void build_agg_plan(const dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in, uint32_t flags,
                    const AggDiag& diag, AggBuilt& B, bool low_sel = false);
void build_batch_plan(const dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in, uint32_t flags,
                      const AggDiag& diag, AggBuilt& B, bool low_sel);
void flush_groups(dfmi_context* ctx, dfmi_agg_state* st);

// ---- agg_batches.cpp: the coalesced entry points
void count_query_launch();  // dfmi_internal_agg_query_launches

// ---- agg_hash.cpp: the device hash table's driver
HashDev& hashdev(dfmi_context* ctx, dfmi_agg_state* st);
void accumulate_hashed(dfmi_context* ctx, dfmi_agg_state* st, const std::vector<dfmi::gb::Col>& cols, int64_t m,
                       const AggDiag& diag, std::chrono::steady_clock::time_point t0);
void group_batch_on_host(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                         uint32_t flags);
void group_batch_hashed(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                        uint32_t flags, const AggDiag& diag);
// ... nb batches (offset-0 columns, fixed-width and Boolean keys and arguments, at most
// gb::kConcatMaxBatches) as one evaluation launch and one run of the table's passes; *failed: the
// first failing batch (the state is failed and the error thrown).
void group_batches_hashed(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins,
                          int32_t nb, uint32_t flags, const AggDiag& diag, int32_t* failed);
void reset_table(dfmi_context* ctx, HashDev& H, const AggDiag& diag);
void unflatten(dfmi_agg_state* st);
void drain_hashed(dfmi_context* ctx, dfmi_agg_state* st);
bool finish_flat(dfmi_context* ctx, dfmi_agg_state* st, const AggDiag& diag);
bool finish_device(dfmi_context* ctx, dfmi_agg_state* st, const AggDiag& diag, int64_t cap, dfmi_agg_value* keys,
                   dfmi_agg_value* values, int64_t* num_groups);
void emit_flat(const dfmi_agg_state* st, const FlatGroups& f, int64_t cap, dfmi_agg_value* keys,
               dfmi_agg_value* values, int64_t* num_groups);
void emit_key_bytes_flat(const FlatGroups& f, int part, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                         int64_t data_capacity, int64_t* data_length);
long bucketed_batches();
long normalize_trips();
long strided_launches();
void read_records(dfmi_context* ctx, dfmi_agg_state* st, uint64_t g0, uint64_t ng, uint64_t* out, int64_t* info);

// ---- agg_strext.cpp: the Utf8 MIN / MAX side structure's driver
void strext_create(dfmi_context* ctx, dfmi_agg_state* st);  // st->sx when the state holds a Utf8 extreme
// one batch's m evaluated rows: cols[j] the argument column of aggregate j (only the Utf8 extremes' are read),
// rg the rows' dense group ids (null: one group), ngroups the groups the device holds
void strext_batch(dfmi_context* ctx, dfmi_agg_state* st, const dfmi::gb::Col* arg_cols, const unsigned* rg, int64_t m,
                  uint64_t ngroups, const AggDiag& diag);
void strext_batch_ungrouped(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                            uint32_t flags, const AggDiag& diag);
// the device side emptied (the last finish's values stay)
void strext_reset(dfmi_context* ctx, dfmi_agg_state* st, const AggDiag& diag);
// the first ng groups' winners and the arena on the host (f.sx_ent, f.sx_arena)
void strext_read(dfmi_context* ctx, dfmi_agg_state* st, FlatGroups& f, uint64_t ng);
void strext_finish_ungrouped(dfmi_context* ctx, dfmi_agg_state* st, dfmi_agg_value* out);
// group g's value of extreme x (StrExt::x index) in a finish's flat groups
dfmi::aggh::StrVal strext_flat_value(const FlatGroups& f, size_t x, uint64_t g);

}  // namespace agg
}  // namespace dfmi
