// The plan of the fused Selection + Projection pass, from the compiled
// predicate / projections (dfmi_program IR): static errors in the reference's
// evaluation order (FilterRelation::next filter.rs:46-72, filter()
// filter.rs:80-111, ProjectRelation::next projection.rs:45-66), output
// metadata, which input columns the kernel loads (predicate columns for every
// row, projection-only columns only where selected), the tile shape with its
// diagnostic knobs, and the selectivity hints that pick between shapes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "launch_args.h"

using namespace dfmi;
using namespace dfmi::xi;

namespace {

// The ring-staged Utf8 gather stages every byte of a 256-row step (not only
// the selected strings), into slots of kRingSlot 16-byte chunks: chosen when
// the same query shape's previous large batch selected at least kRingSel of
// its rows and its selected strings averaged at most kRingLen bytes (a step
// then fits a slot with ~10% to spare; a longer step copies per lane).
constexpr int kRingSlot = 256;
constexpr double kRingSel = 0.15;
constexpr double kRingLen = 14.5;
constexpr double kLongLen = 24.0;  // selected Utf8 bytes per row from which slices tend to overflow the 2 KiB stage
constexpr bool kRingDefault = false;

// A numeric predicate over a large batch that selects few rows runs the
// sub-tile kernel: M sub-tiles of BLOCK * K rows share one scan + look-back
// (one look-back per 16,384 rows instead of per 4,096), the predicate pass
// keeps only selection ballots, and the output pass reloads just the columns
// the outputs read, for the selected rows (jit_kernels.cpp "M sub-tiles"). Chosen
// from the selectivity the same query shape had on its previous large batch
// on this context (below kLowSel); the first call, and any call after a
// batch selected more, runs the one-tile kernel, which keeps every loaded
// value in registers across the look-back.
constexpr int64_t kSubtileMinRows = (int64_t)1 << 22;
constexpr double kLowSel = 0.04;

// The tile shape of the plan's kernel, before any diagnostic knob.
void choose_tile_shape(jit::Launch& X, const dfmi_program* pred, int64_t n, const Built& B) {
    // rows per thread: keep the tile's column data resident in VGPRs (a
    // Utf8 column holds its offsets per row; a kernel gathering many Utf8
    // columns at K = 8 is also a ~35 s hipRTC compile -- 11 Utf8 outputs:
    // 35 / 15 / 6.6 s at K = 8 / 4 / 2)
    const size_t nload = X.num_cols.size() + X.utf8_cols.size();
    X.BLOCK = 512;
    X.K = nload <= 4 ? 8 : (nload <= 8 ? 4 : 2);
    // a predicate over Utf8 columns only reads ~4 B/row of offsets: its tiles
    // are latency-bound, and 4-wave blocks keep more of them resident
    // (C3 equality 4.94 -> 4.53 ms)
    // (... unless the same query selected >= kLowSel of a large batch last
    // time -- `s != 'w17...'`, 99.9%: the one-tile kernel with the LDS-image
    // gather below, 2.37 -> 1.63 ms per C3 batch; profiles/r05/c3_ne_probe*.log)
    if (pred && X.pred_slots.empty() && !X.utf8_cols.empty() && !B.high_sel) {
        X.BLOCK = 256;
        // ... and are latency-bound on the look-back: a 16-predecessor poll
        // window and 8 waves/SIMD (a few spilled registers) measured faster
        // (C3 equality 0.826 -> 0.675 ms per 1.25e8-row batch)
        X.window = 16;
        X.waves_per_eu = 8;
        // ... and M sub-tiles share one look-back, their output pass two
        // slices per wave at a time: 60 VGPRs, no spills at 8 waves/SIMD
        // (DESIGN.md §4 "Sub-tiles")
        X.M = 8;
        X.KO = 2;
    } else {
        // Utf8 outputs of a numeric predicate: the LDS-image gather (the
        // binary-search emitter's smaller LDS footprint only pays where few
        // rows are selected)
        X.gather = 4;
        if (!X.utf8_outs.empty() && pred) {
            // latency-bound gather: a 2 KiB staging arena per wave, 256-thread
            // blocks and a soft occupancy hint (a shape that would spill at it
            // is compiled again without it)
            X.arena = 128;
            X.waves_soft = true;
            // ... 61 VGPRs since the light fallback copy: 8 waves/SIMD fit
            // without spills (256-thread blocks: 1.045 -> 1.021 ms per C3
            // batch; 7 waves and 72 VGPRs were the budget of utf8_copy's
            // 8-word chunks; profiles/r05/c3_combo.log) ...
            X.waves_per_eu = 8;
            // ... where 512-thread blocks (4096-row tiles: half the look-backs)
            // beat 256 with a 12-predecessor window: 1.076 -> 1.032-1.042 ms
            // same box (1024: 1.087-1.096; windows 4 / 8 / 12 / 32 at 512:
            // 1.077 / 1.036-1.042 / 1.032 / 1.061; profiles/r05/c3_block_ab.log)
            X.BLOCK = 512;
            X.window = 12;
            // ... and where the last large batch selected long strings (slices
            // over the stage), the per-lane fallback with 64 bytes in flight
            // and no occupancy hint (81 VGPRs): 40-200-byte strings 1.29 ->
            // 0.79 ms per 1e7 rows (profiles/r05/long_utf8_copy.log)
            if (B.long_utf8) {
                X.long_copy = 1;
                X.waves_per_eu = 0;
            }
            // ... at high selectivity, the ring-staged gather (one loader wave)
            // when kRingDefault: same-box A/B (profiles/r05/c3_ring_ab.log) put it
            // within the box's spread of the per-wave gather (1.135-1.153 vs
            // 1.138-1.143 ms per C3 batch), so it stays a diagnostic variant
            if (kRingDefault && B.ring_ok && X.utf8_outs.size() == 1 && !X.pred_slots.empty()) {
                X.ring = kRingSlot;
                X.BLOCK = 256;  // a ring step = one 64-row slice per wave of 4
                X.window = 16;
            }
        } else if (pred && B.low_sel && !X.pred_slots.empty() && X.utf8_cols.empty() && n >= kSubtileMinRows) {
            // a numeric predicate that selected < 4% last time: M sub-tiles
            // share one look-back, a sparse output pass re-reads only the
            // selected rows (same-box A/B, profiles/r04/ab_subtiles*.log: C2
            // s = 1% (2 predicate columns) 4.17 / 3.12 / 3.00 / 3.03 ms and C4
            // (4) 3.01 / 2.76 / 2.60 / 2.51 ms at M = 1 / 8 / 4 / 2: more
            // predicate registers per sub-tile, fewer sub-tiles)
            X.BLOCK = 256;
            X.M = X.pred_slots.size() >= 3 ? 2 : 4;
            X.KO = 2;  // the (rare) dense output pass two slices at a time: fewer registers
        }
    }
}

// The diagnostic knobs (tools/*): read only when DFMI_DIAG is set -- a dozen
// getenv scans per call would cost the 1024-row batch path microseconds. In
// this order: several read what earlier ones set.
void apply_diag_knobs(jit::Launch& X, const dfmi_program* pred) {
    if (const char* kk = getenv("DFMI_ROWS_PER_THREAD")) X.K = atoi(kk);
    if (const char* bb = getenv("DFMI_BLOCK")) X.BLOCK = atoi(bb);
    if (const char* ww = getenv("DFMI_WAVES_PER_EU")) X.waves_per_eu = atoi(ww);
    // look-back / tile-order variants
    if (const char* e = getenv("DFMI_LOOKBACK_R")) X.R = std::max(1, std::min(16, atoi(e)));
    if (const char* e = getenv("DFMI_LOOKBACK_SLEEP")) X.sleep = std::max(0, std::min(127, atoi(e)));
    if (const char* e = getenv("DFMI_LOOKBACK_SPREAD")) X.spread = std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("DFMI_LOOKBACK_W")) X.window = std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("DFMI_NT")) X.nt = atoi(e) & 3;
    if (const char* e = getenv("DFMI_UTF8_PRESTAGE")) X.prestage = atoi(e) & 3;  // 2: not the look-back wave
    if (const char* e = getenv("DFMI_GATHER_PHASES")) X.gather_phases = atoi(e) & 1;
    if (const char* e = getenv("DFMI_UTF8_GATHER")) X.gather = atoi(e) % 7;  // 2 = serial, 3 = two-pass, 4 = LDS image, 5 = marker scan, 6 = direct
    if (const char* e = getenv("DFMI_UTF8_DIRECT_GROUP")) X.direct_grp = atoi(e);
    if (const char* e = getenv("DFMI_LATE_PROJ")) X.late_proj = atoi(e) & 1;
    if (const char* e = getenv("DFMI_PROJ_DENSE")) X.proj_dense = atoi(e) & 1;
    if (const char* e = getenv("DFMI_TICKET")) X.ticket = atoi(e) & 1;  // ticket-ordered tiles from the start
    if (const char* e = getenv("DFMI_UTF8_EARLY")) X.early = atoi(e) & 1;
    if (const char* e = getenv("DFMI_LIGHT_COPY")) X.light_copy = atoi(e) & 1;
    if (const char* e = getenv("DFMI_LONG_COPY")) X.long_copy = atoi(e) & 3;  // 1: per lane, 2: wave-cooperative
    if (const char* e = getenv("DFMI_UTF8_EQ_DENSE")) {  // chunks of the per-wave arena (dense equality A/B)
        X.eq_dense = std::max(0, std::min(1024, atoi(e)));
        if (X.eq_dense) X.waves_per_eu = 0;  // LDS-limited occupancy: no register hint
    }
    if (const char* e = getenv("DFMI_UTF8_EQ_REG")) {  // register-resident dense equality: G slices per round
        const int g = atoi(e);
        if (g == 1 || g == 2 || g == 4 || g == 8) X.eq_dense = X.K % g == 0 ? -g : 0;
    }
    // Utf8 ordering compares: head width, and the tile pre-pass off (per-row helper in the loop)
    if (const char* e = getenv("DFMI_UTF8_ORD_H")) X.ord_h = atoi(e) == 8 ? 8 : 4;
    if (const char* e = getenv("DFMI_UTF8_ORD_PRE")) X.ord_pre = atoi(e) & 1;
    if (const char* e = getenv("DFMI_UTF8_RING"))  // 0: off; > 0: on (slot chunks) where it applies
        if (pred && X.utf8_outs.size() == 1 && !X.pred_slots.empty() && X.M == 1) {
            X.ring = atoi(e) > 1 ? atoi(e) : (atoi(e) == 1 ? kRingSlot : 0);
            if (X.ring) {  // a step = one 64-row slice per wave of 4
                X.BLOCK = 256;
                X.window = 16;
            }
        }
    if (const char* e = getenv("DFMI_SUBTILES"))
        if (X.pred_slots.empty() && !X.utf8_cols.empty()) X.M = std::max(1, std::min(32, atoi(e)));
    // the numeric sub-tile kernel at any size (parity tests, A/B runs)
    // (1: the one-tile kernel even where the selectivity hint picks sub-tiles)
    if (const char* e = getenv("DFMI_NUMERIC_SUBTILES"))
        if (pred && !X.pred_slots.empty() && X.utf8_cols.empty()) {
            X.BLOCK = atoi(e) > 1 ? 256 : 512;
            X.M = std::max(1, std::min(8, atoi(e)));
            X.KO = X.M > 1 ? 2 : 0;
        }
    if (const char* e = getenv("DFMI_OUT_SLICES")) X.KO = atoi(e);
    if (const char* e = getenv("DFMI_SUBTILE_PREFETCH")) X.prefetch = atoi(e) & 1;
    if (const char* e = getenv("DFMI_SUBTILE_SPARSE")) X.sparse = atoi(e) & 1;
    if (const char* e = getenv("DFMI_UTF8_ARENA")) X.arena = std::max(128, std::min(1024, atoi(e)));
    if (const char* e = getenv("DFMI_UTF8_IMAGE")) X.image = std::max(32, std::min(129, atoi(e)));
    if (const char* e = getenv("DFMI_UTF8_DBUF")) X.dbuf = atoi(e) & 1;
    if (const char* e = getenv("DFMI_UTF8_ST16")) X.st16 = atoi(e) & 1;
    if (const char* e = getenv("DFMI_UTF8_PAIRS")) {
        X.pairs = atoi(e) & 1;
        if (X.pairs) X.image = 130;  // two images of 65 chunks
    }
}

// The whole plan: checks, static errors, output plan, slots, tile shape.
void build_plan_impl(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch* in,
                     dfmi_out_column* outs, uint32_t flags, Built& B) {
    Err& se = B.se;
    jit::Plan& plan = B.plan;
    jit::Launch& X = B.X;
    bool& any_kernel_out = B.any_kernel_out;
    const int64_t n = in->num_rows;
    const int ncols = in->num_columns;
    if (pred) check_schema(pred, in);
    for (int j = 0; j < np; ++j) {
        if (!projs[j]) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL projection"};
        check_schema(projs[j], in);
    }
    check_not_ragged(in);

    // ---- errors every evaluation of this plan raises (reference order)
    std::vector<int> proj_base(np);
    int base = offer_filter_errors(pred, in, flags, se);
    for (int j = 0; j < np; ++j) {
        proj_base[j] = base;
        offer_program_errors(projs[j], base, se);
        base += projs[j]->length;
    }
    check_ordinal_limit(base);

    // ---- output plan
    const int nout = np > 0 ? np : ncols;
    if (nout > 16) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device program limit: too many output columns"};
    plan.pred = pred;
    plan.outs.resize(nout);
    X.in = in;
    for (int o = 0; o < nout; ++o) {
        dfmi_out_column& oc = outs[o];
        const dfmi_program* p = np > 0 ? projs[o] : nullptr;
        const IrNode* root = p ? &p->ir[p->root] : nullptr;
        const bool is_col = !p || root->kind == IR_COL;
        const int col = p ? root->col : o;
        oc.type = p ? p->type : in->columns[o].type;
        oc.passthrough_column = -1;
        oc.length = 0;
        oc.null_count = 0;
        oc.data_length = 0;
        jit::OutSpec& os = plan.outs[o];
        os.out_type = oc.type;
        if (is_col && !pred) {  // Arc clone of the input column (expression.rs:274)
            const dfmi_column& c = in->columns[col];
            oc.passthrough_column = col;
            oc.length = n;
            oc.null_count = c.validity ? c.null_count : 0;
            continue;
        }
        if (is_col) {
            const int ct = in->columns[col].type;
            if (!gatherable(ct, flags)) continue;  // error raised at ordinal P+1
            if (ct == DFMI_TYPE_UTF8) {
                if (!oc.offsets || !oc.data) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "Utf8 output buffers are NULL"};
                os.kind = jit::OutSpec::UTF8;
            } else {
                if (!oc.values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "output values pointer is NULL"};
                os.kind = jit::OutSpec::GATHER;
            }
            os.col = col;
            any_kernel_out = true;
            continue;
        }
        if (oc.type == DFMI_TYPE_UTF8) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "device path: Utf8-valued projection"};
        if (!oc.values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "output values pointer is NULL"};
        os.kind = jit::OutSpec::EXPR;
        os.prog = p;
        os.ord_base = proj_base[o];
        os.nullable = pred && jit::may_introduce_nulls(p);
        if (os.nullable && !oc.validity)
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "output validity pointer is NULL (the projection can produce nulls)"};
        any_kernel_out = true;
    }

    // ---- column slots: predicate columns first, then projection-only ones
    Slots slots{X};
    if (pred) slots.prog(pred, X.pred_slots);
    for (int o = 0; o < nout; ++o) {
        const jit::OutSpec& os = plan.outs[o];
        if (os.kind == jit::OutSpec::GATHER) slots.num(os.col, X.proj_slots);
        else if (os.kind == jit::OutSpec::EXPR) slots.prog(os.prog, X.proj_slots);
        else if (os.kind == jit::OutSpec::UTF8) X.utf8_outs.push_back({o, slots.utf8(os.col)});
    }
    slots.check_limit(kArgCols, kArgUtf8);

    choose_tile_shape(X, pred, n, B);
    if (getenv("DFMI_DIAG")) apply_diag_knobs(X, pred);
    if (X.dbuf && X.arena < 128) X.dbuf = 0;  // halves of >= 64 chunks (longer spans copy per lane)
    if (X.M == 1 || X.KO == 0) X.KO = X.K;
    if (X.direct_grp < 1) X.direct_grp = 1;
    while (X.K % X.direct_grp || X.KO % X.direct_grp) X.direct_grp >>= 1;  // divides the slices it groups
    if (X.KO < 1 || X.KO > X.K || X.K % X.KO) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad tile shape"};
    if (X.K < 1 || X.K > 32 || X.BLOCK < 64 || X.BLOCK > 1024 || X.BLOCK % 64 || X.K * X.M * X.BLOCK / 64 > 256)
        throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad tile shape"};
    B.n_tiles = tiles_of(n, (int64_t)X.BLOCK * X.K * X.M);
    // a filtered batch with one Utf8 output packs rows and bytes into one
    // 62-bit look-back word (31 + 31 bits, jit_skeleton.hip tile_scan_publish)
    if (X.utf8_outs.size() == 1 && n >= (int64_t(1) << 31))
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "batch too large"};
}

// The selectivity hint's key: the programs and the batch's column types /
// nullability (a performance hint only: results never depend on it).
uint64_t sel_hint_key(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch* in,
                      uint32_t flags) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix((uint64_t)(uintptr_t)pred);
    mix((uint64_t)np);
    for (int j = 0; j < np; ++j) mix((uint64_t)(uintptr_t)projs[j]);
    mix(flags);
    for (int i = 0; i < in->num_columns; ++i)
        mix((uint64_t)in->columns[i].type << 1 | (in->columns[i].validity && in->columns[i].null_count > 0));
    return h;
}

}  // namespace

void dfmi::xi::build_plan(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np,
                          const dfmi_batch* in, dfmi_out_column* outs, uint32_t flags, Built& B) {
    static_error_first(B.se, [&] { build_plan_impl(pred, projs, np, in, outs, flags, B); });
}

uint64_t dfmi::xi::sel_hint_lookup(const dfmi_context* ctx, const dfmi_program* pred,
                                   const dfmi_program* const* projs, int32_t np, const dfmi_batch* in,
                                   uint32_t flags, Built& B) {
    if (!pred || in->num_rows < kSubtileMinRows) return 0;
    const uint64_t key = sel_hint_key(pred, projs, np, in, flags);
    const auto it = ctx->sel_hint.find(key);
    B.low_sel = it != ctx->sel_hint.end() && it->second < kLowSel;
    B.high_sel = it != ctx->sel_hint.end() && it->second >= kLowSel;
    const auto lt = ctx->utf8_len_hint.find(key);
    B.ring_ok = it != ctx->sel_hint.end() && it->second >= kRingSel && lt != ctx->utf8_len_hint.end() &&
                lt->second <= kRingLen;
    B.long_utf8 = lt != ctx->utf8_len_hint.end() && lt->second >= kLongLen;
    return key;
}

void dfmi::xi::sel_hint_update(dfmi_context* ctx, uint64_t key, const jit::Launch& X, int64_t n, int64_t out_rows,
                               uint64_t utf8_bytes) {
    if (ctx->sel_hint.size() >= 4096) ctx->sel_hint.clear();
    ctx->sel_hint[key] = (double)out_rows / (double)n;
    if (!X.utf8_outs.empty() && out_rows > 0) {
        if (ctx->utf8_len_hint.size() >= 4096) ctx->utf8_len_hint.clear();
        ctx->utf8_len_hint[key] = (double)utf8_bytes / (double)out_rows;
    }
}

// Internal test hook (not part of the C ABI, not declared in include/):
// generates the query kernel a dfmi_filter_project call would launch and, if
// compile != 0, compiles it with hipRTC -- no device needed, so the CPU test
// suite checks code generation for every expression shape it covers.
// Returns the source length (the text is truncated to cap), or -status.
// Flag bit 0x40000000: the coalesced-batches form; 0x20000000: the shape
// chosen after the query's last large batch selected most rows (high_sel).
extern "C" int64_t dfmi_internal_jit_check(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np,
                                           const dfmi_batch* in, dfmi_out_column* outs, uint32_t flags,
                                           int32_t compile, char* buf, int64_t cap, dfmi_error* err) {
    return guarded_size(err, [&]() -> int64_t {
        if (!in || (np > 0 && !projs) || !outs) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
        Built B;
        B.high_sel = (flags & 0x20000000u) != 0;  // as if the query's last large batch selected most rows
        build_plan(pred, projs, np, in, outs, flags & ~0x60000000u, B);
        B.X.batched = (flags & 0x40000000u) != 0;  // the coalesced-batches form of the kernel
        const std::string src = jit::generate(B.plan, B.X);
        if (compile) (void)jit::compile_code(src, nullptr);
        if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", src.c_str());
        return (int64_t)src.size();
    });
}
