// Aggregate extension, MIN / MAX over a Utf8 argument
// (DFMI_FLAG_EXT_AGG_MINMAX_ANY): the driver of the string side structure
// (str_extreme.h; kernels in str_extreme.hip). Inside the record machinery
// such an aggregate is a COUNT (agg_host.h acc_fn); here, per batch, the
// evaluated argument column and the rows' dense group ids go through the
// prefix, candidate and keep passes, and a finish reads the persisted winners
// back beside the records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "agg_state.h"

using namespace dfmi;
using namespace dfmi::xi;
using namespace dfmi::aggh;

namespace dfmi {
namespace agg {

namespace {

constexpr uint64_t kArena0 = 1 << 16;

// The side arrays hold (initialised) at least `ng` groups.
void ensure_groups(dfmi_context* ctx, StrExt& S, uint64_t ng, int grid) {
    if (ng <= S.gcap) return;
    uint64_t want = std::max<uint64_t>(S.gcap, 1);
    while (want < ng) want *= 2;
    for (StrExt::One& o : S.x) {
        o.pref.regrow(ctx->stream, S.gcap * 8, want * 8);
        o.best.regrow(ctx->stream, S.gcap * 4, want * 4);
        o.ent.regrow(ctx->stream, S.gcap * sizeof(sx::Ent), want * sizeof(sx::Ent));
        HIP_TRY(sx::launch_init(o.pref.as<unsigned long long>(), o.best.as<unsigned>(), o.ent.as<sx::Ent>(), o.is_min, S.gcap,
                                want, grid, ctx->stream));
    }
    S.gcap = want;
}

// The bytes an evaluated Utf8 column of m rows holds.
uint64_t column_bytes(dfmi_context* ctx, const int32_t* offsets, int64_t m) {
    int32_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], offsets, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&ends[1], offsets + m, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return (uint64_t)std::max(0, ends[1] - ends[0]);
}

// The device header on the host (synchronises the stream).
sx::Hdr read_hdr(dfmi_context* ctx, StrExt& S) {
    sx::Hdr h{};
    HIP_TRY(hipMemcpyAsync(&h, S.hdr.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return h;
}

// Room for `need` more bytes behind arena_end. Superseded strings do not
// accumulate: when the arena is full its live strings (Hdr::live bytes) are
// compacted straight into a fresh one, a power of two in which live + need
// fill at most half -- so the arena holds at most four times the winners'
// bytes plus what one batch keeps, and shrinks again when they do.
void ensure_arena(dfmi_context* ctx, StrExt& S, uint64_t ng, uint64_t need, int grid) {
    if (S.arena_end + need <= S.arena_cap) return;
    uint64_t cap = kArena0;
    while (cap < 2 * (S.live + need)) cap *= 2;
    DevBuf fresh;
    fresh.alloc(cap);
    HIP_TRY(hipMemsetAsync(&S.hdr.as<sx::Hdr>()->arena_end, 0, 8, ctx->stream));
    // all extremes share the arena: each compacts its strings behind the last one's
    for (StrExt::One& o : S.x)
        HIP_TRY(sx::launch_compact(o.ent.as<sx::Ent>(), std::min(ng, S.gcap), S.arena.as<unsigned char>(),
                                   fresh.as<unsigned char>(), cap, S.hdr.as<sx::Hdr>(), grid, ctx->stream));
    const sx::Hdr h = read_hdr(ctx, S);
    if (h.arena_end != S.live) throw Fail{DFMI_ERR_DEVICE, "Utf8 MIN / MAX: the string arena's live bytes do not add up"};
    S.arena = std::move(fresh);  // (the old arena goes with the local)
    S.arena_cap = cap;
    S.arena_end = h.arena_end;
}

}  // namespace

void strext_create(dfmi_context* ctx, dfmi_agg_state* st) {
    if (!any_utf8_extreme(st->aggs.data(), st->aggs.size())) return;
    auto S = std::make_unique<StrExt>();
    for (size_t j = 0; j < st->aggs.size(); ++j)
        if (is_utf8_extreme(*st->aggs[j])) {
            StrExt::One o;
            o.agg = (int)j;
            o.is_min = st->aggs[j]->fn == DFMI_AGG_MIN;
            S->x.push_back(std::move(o));
        }
    S->hdr.alloc(sizeof(sx::Hdr));
    HIP_TRY(hipMemsetAsync(S->hdr.p, 0, sizeof(sx::Hdr), ctx->stream));
    S->arena.alloc(kArena0);
    S->arena_cap = kArena0;
    S->one.assign(st->aggs.size(), StrVal{});
    ensure_groups(ctx, *S, st->grouped ? 1024 : 1, group_grid(agg_diag()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st->sx = std::move(S);
}

// The device side emptied: no group holds a winner (a reset, or a drain of the
// table whose group ids these arrays follow). What the last finish produced
// (StrExt::one, finished) is the caller's to keep or drop.
void strext_reset(dfmi_context* ctx, dfmi_agg_state* st, const AggDiag& diag) {
    if (!st->sx) return;
    StrExt& S = *st->sx;
    if (S.arena_cap > kArena0) {  // (a large batch's arena is not kept for the state's lifetime)
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        S.arena.alloc(kArena0);
        S.arena_cap = kArena0;
    }
    for (StrExt::One& o : S.x)
        HIP_TRY(sx::launch_init(o.pref.as<unsigned long long>(), o.best.as<unsigned>(), o.ent.as<sx::Ent>(), o.is_min, 0, S.gcap,
                                group_grid(diag), ctx->stream));
    HIP_TRY(hipMemsetAsync(S.hdr.p, 0, sizeof(sx::Hdr), ctx->stream));
    S.arena_end = S.live = 0;
}

void strext_batch(dfmi_context* ctx, dfmi_agg_state* st, const dfmi::gb::Col* arg_cols, const unsigned* rg, int64_t m,
                  uint64_t ngroups, const AggDiag& diag) {
    if (!st->sx || m <= 0 || !ngroups) return;
    StrExt& S = *st->sx;
    const int grid = group_grid(diag);
    ensure_groups(ctx, S, ngroups, grid);
    auto args = [&](const StrExt::One& o) {
        const dfmi::gb::Col& c = arg_cols[o.agg];
        sx::Args a{};
        a.bytes = (const unsigned char*)c.values;
        a.offsets = c.offsets;
        a.validity = c.validity;
        a.rg = rg;
        a.m = m;
        a.is_min = o.is_min ? 1 : 0;
        a.ngroups = ngroups;
        a.pref = o.pref.as<unsigned long long>();
        a.best = o.best.as<unsigned>();
        a.ent = o.ent.as<sx::Ent>();
        a.arena = S.arena.as<unsigned char>();
        a.arena_cap = S.arena_cap;
        a.hdr = S.hdr.as<sx::Hdr>();
        return a;
    };
    // the batch's winners found and their bytes measured; then exactly that much room; then kept
    HIP_TRY(hipMemsetAsync(&S.hdr.as<sx::Hdr>()->need, 0, 8, ctx->stream));
    for (const StrExt::One& o : S.x) HIP_TRY(sx::launch_find(args(o), grid, ctx->stream));
    ensure_arena(ctx, S, ngroups, read_hdr(ctx, S).need, grid);
    for (const StrExt::One& o : S.x) HIP_TRY(sx::launch_keep(args(o), grid, ctx->stream));
    const sx::Hdr h = read_hdr(ctx, S);
    S.arena_end = h.arena_end;
    S.live = h.live;
    if (S.arena_end > S.arena_cap) throw Fail{DFMI_ERR_DEVICE, "Utf8 MIN / MAX: the string arena overflowed"};
}

// An ungrouped batch (after its fused kernel, in which the Utf8 extremes
// counted): the Utf8 arguments evaluated once through the Selection +
// Projection pass with the same predicate (a pass-through without one), then
// the passes with every row in group 0.
void strext_batch_ungrouped(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                            uint32_t flags, const AggDiag& diag) {
    if (!st->sx || in->num_rows <= 0) return;
    StrExt& S = *st->sx;
    const size_t nx = S.x.size();
    const int64_t rows = in->num_rows;
    std::vector<const dfmi_program*> progs(nx);
    std::vector<dfmi_out_column> outs(nx);
    if (S.eval.size() < 3 * nx) S.eval.resize(3 * nx);
    for (size_t q = 0; q < nx; ++q) {
        progs[q] = &st->aggs[S.x[q].agg]->arg;
        dfmi_out_column& c = outs[q];
        memset(&c, 0, sizeof c);
        const IrNode& root = progs[q]->ir[progs[q]->root];
        size_t cap = 8;
        if (root.kind == IR_COL && root.col >= 0 && root.col < in->num_columns && in->columns[root.col].offsets) {
            cap = std::max<size_t>(cap, (size_t)column_bytes(ctx, in->columns[root.col].offsets, rows));
        }
        c.offsets = (int32_t*)S.eval[3 * q].reserve((size_t)(rows + 1) * 4);
        c.data = (uint8_t*)S.eval[3 * q + 1].reserve(cap);
        c.data_capacity = (int64_t)cap;
        c.validity = (uint8_t*)S.eval[3 * q + 2].reserve((size_t)(rows + 63) / 64 * 8);
    }
    dfmi_error e{};
    if (dfmi_filter_project(ctx, pred, progs.data(), (int32_t)nx, in, outs.data(), flags, &e) != DFMI_OK) {
        st->failed = true;
        st->failure = e;
        throw Fail{e.code, e.message};
    }
    std::vector<dfmi::gb::Col> cols(st->aggs.size(), dfmi::gb::Col{});
    for (size_t q = 0; q < nx; ++q) {
        const dfmi_out_column& c = outs[q];
        dfmi::gb::Col& d = cols[S.x[q].agg];
        d.type = DFMI_TYPE_UTF8;
        if (c.passthrough_column >= 0) {
            const dfmi_column& src = in->columns[c.passthrough_column];
            d.values = src.values;
            d.offsets = src.offsets;
            d.validity = src.null_count > 0 ? src.validity : nullptr;
        } else {
            d.values = c.data;
            d.offsets = c.offsets;
            d.validity = c.null_count > 0 ? c.validity : nullptr;
        }
    }
    strext_batch(ctx, st, cols.data(), nullptr, outs[0].length, 1, diag);
}

void strext_read(dfmi_context* ctx, dfmi_agg_state* st, FlatGroups& f, uint64_t ng) {
    f.sx_ent.clear();
    f.sx_arena.clear();
    if (!st->sx) return;
    StrExt& S = *st->sx;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    f.sx_ent.resize(S.x.size());
    const uint64_t have = std::min(ng, S.gcap);
    for (size_t q = 0; q < S.x.size(); ++q) {
        sx::Ent none{};
        none.len = sx::kNone;
        f.sx_ent[q].assign((size_t)ng, none);
        if (have) HIP_TRY(hipMemcpy(f.sx_ent[q].data(), S.x[q].ent.p, have * sizeof(sx::Ent), hipMemcpyDeviceToHost));
    }
    f.sx_arena.resize((size_t)S.arena_end);
    if (S.arena_end) HIP_TRY(hipMemcpy(f.sx_arena.data(), S.arena.p, (size_t)S.arena_end, hipMemcpyDeviceToHost));
}

StrVal strext_flat_value(const FlatGroups& f, size_t x, uint64_t g) {
    StrVal v;
    if (x >= f.sx_ent.size() || g >= f.sx_ent[x].size()) return v;
    const sx::Ent& e = f.sx_ent[x][(size_t)g];
    if (e.len == sx::kNone || e.off + e.len > f.sx_arena.size()) return v;
    v.has = true;
    v.s.assign((const char*)f.sx_arena.data() + e.off, e.len);
    return v;
}

// The ungrouped finish: out[j] of a Utf8 extreme gets its byte length; the
// bytes stay in S.one for dfmi_agg_state_value_bytes.
void strext_finish_ungrouped(dfmi_context* ctx, dfmi_agg_state* st, dfmi_agg_value* out) {
    if (!st->sx) return;
    StrExt& S = *st->sx;
    FlatGroups f;
    strext_read(ctx, st, f, 1);
    for (size_t q = 0; q < S.x.size(); ++q) {
        const int j = S.x[q].agg;
        S.one[j] = out[j].is_null ? StrVal{} : strext_flat_value(f, q, 0);
        if (!out[j].is_null) out[j].bits = S.one[j].s.size();
    }
    S.finished = true;
}

}  // namespace agg
}  // namespace dfmi
