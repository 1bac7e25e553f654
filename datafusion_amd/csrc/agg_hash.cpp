// Aggregate extension: the driver of the device hash table (groupby.h; kernels
// in groupby.hip) -- several GROUP BY keys, a float or Utf8 key, or integer
// keys wider than the key window. Per batch: the fused evaluation pass, the
// claim pass, the accumulate pass (scattered or bucketed); at a finish or a
// drain: the groups read out flat, ordered and emitted on the host or on the
// device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "agg_state.h"
#include "batch_stage.h"
#include "jit_skeleton.hip"

using namespace dfmi;
using namespace dfmi::xi;
using namespace dfmi::aggh;

// agg_host.h restates the accumulator layout for the host-only code.
static_assert(layout::kAggCopies == kAggCopies && layout::kAggLimbs == kAggLimbs && layout::kAggWords == kAggWords,
              "agg_host.h layout as jit_skeleton.hip");
static_assert((unsigned)layout::AGGF_NAN == AGGF_NAN && (unsigned)layout::AGGF_PINF == AGGF_PINF &&
                  (unsigned)layout::AGGF_NINF == AGGF_NINF && (unsigned)layout::AGGF_NONNEGZERO == AGGF_NONNEGZERO &&
                  (unsigned)layout::AGGF_VALUE == AGGF_VALUE,
              "agg_host.h flags as jit_skeleton.hip");
static_assert(layout::kRoundZero == gb::kRoundZero && layout::kMaxKeys == gb::kMaxKeys, "agg_host.h as groupby.h");

namespace dfmi {
namespace agg {
namespace {

constexpr uint64_t kTableSlots0 = 1 << 16;

// A table of `cap` slots, its control words zeroed on the stream.
void alloc_table(DevBuf& ctl, DevBuf& slot, gb::Table& t, uint64_t cap, hipStream_t stream) {
    ctl.alloc(cap * 8);
    slot.alloc(cap * sizeof(gb::Slot));
    HIP_TRY(hipMemsetAsync(ctl.p, 0, cap * 8, stream));
    t = gb::Table{};
    t.ctl = ctl.as<unsigned long long>();
    t.slot = slot.as<gb::Slot>();
    t.mask = cap - 1;
}

}  // namespace

HashDev& hashdev(dfmi_context* ctx, dfmi_agg_state* st) {
    if (st->hd) return *st->hd;
    auto H = std::make_unique<HashDev>();
    const size_t n = st->aggs.size();
    int w = 1;  // word 0: the group's rows
    for (size_t j = 0; j < n; ++j) {
        H->off.push_back(w);
        const bool fs = acc_fn(*st->aggs[j]) == DFMI_AGG_SUM && is_float_type(st->aggs[j]->arg.type);
        if (fs) H->foff.push_back(w + 4);
        w += 4 + (fs ? kAggLimbs : 0);
    }
    H->words = w;
    H->hpattern.assign((size_t)w, 0);
    for (size_t j = 0; j < n; ++j)
        if (st->aggs[j]->fn == DFMI_AGG_MIN) H->hpattern[(size_t)H->off[j] + 2] = ~0ull;
    H->pattern.alloc((size_t)w * 8);
    HIP_TRY(hipMemcpyAsync(H->pattern.p, H->hpattern.data(), (size_t)w * 8, hipMemcpyHostToDevice, ctx->stream));
    H->hdr.alloc(sizeof(gb::Hdr));
    HIP_TRY(hipMemsetAsync(H->hdr.p, 0, sizeof(gb::Hdr), ctx->stream));
    H->hh.resize(1);
    H->cap = kTableSlots0;
    alloc_table(H->ctl, H->slot, H->t, H->cap, ctx->stream);
    H->acc_cap = 1024;
    H->acc.alloc(H->acc_cap * (size_t)w * 8);
    HIP_TRY(gb::launch_init(H->records(), H->pattern.as<unsigned long long>(), w, 0, H->acc_cap, group_grid(agg_diag()),
                            ctx->stream));
    H->arena_cap = 1 << 16;
    H->arena.alloc(H->arena_cap);
    st->hd = std::move(H);
    return *st->hd;
}

namespace {

void read_hdr(dfmi_context* ctx, HashDev& H) {
    HIP_TRY(hipMemcpyAsync(H.hh.p, H.hdr.p, sizeof(gb::Hdr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// A bigger table (cap x 4), every used slot moved (k_group_rehash).
void grow_table(dfmi_context* ctx, HashDev& H, int grid) {
    DevBuf ctl, slot;
    gb::Table nt;
    const uint64_t ncap = H.cap * 4;
    alloc_table(ctl, slot, nt, ncap, ctx->stream);
    HIP_TRY(gb::launch_rehash(H.t, nt, grid, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    H.ctl = std::move(ctl);  // (the old table goes with the locals)
    H.slot = std::move(slot);
    H.t = nt;
    H.cap = ncap;
}

// ---- the fused evaluation pass of a grouped batch: keys then arguments,
// compacted by the predicate (dfmi_filter_project: the reference's
// evaluation order and first error), into the hash state's reusable device
// buffers. Returns the selected rows; `cols` describes each output (a
// passed-through input column, or the compacted output).
int64_t eval_grouped(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                     uint32_t flags, std::vector<dfmi::gb::Col>& cols) {
    HashDev& H = hashdev(ctx, st);
    const size_t nk = st->keys.size(), n = st->aggs.size();
    const int no = (int)(nk + n);
    const int64_t rows = in->num_rows;
    std::vector<const dfmi_program*> progs(no);
    for (size_t p = 0; p < nk; ++p) progs[p] = &st->keys[p];
    for (size_t j = 0; j < n; ++j) progs[nk + j] = &st->aggs[j]->arg;
    std::vector<dfmi_out_column> outs(no);
    size_t bi = 0;
    for (int o = 0; o < no; ++o) {
        dfmi_out_column& c = outs[o];
        memset(&c, 0, sizeof c);
        const int t = progs[o]->type;
        if (t == DFMI_TYPE_UTF8) {
            const IrNode& root = progs[o]->ir[progs[o]->root];
            size_t cap = 8;
            if (root.kind == IR_COL && root.col >= 0 && root.col < in->num_columns && in->columns[root.col].offsets) {
                int32_t ends[2] = {0, 0};
                HIP_TRY(hipMemcpyAsync(&ends[0], in->columns[root.col].offsets, 4, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(hipMemcpyAsync(&ends[1], in->columns[root.col].offsets + rows, 4, hipMemcpyDeviceToHost,
                                       ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                cap = std::max<size_t>(cap, (size_t)std::max(0, ends[1] - ends[0]));
            }
            c.offsets = (int32_t*)H.bufs[HashDev::EvalOut + bi++].reserve((size_t)(rows + 1) * 4);
            c.data = (uint8_t*)H.bufs[HashDev::EvalOut + bi++].reserve(cap);
            c.data_capacity = (int64_t)cap;
        } else {
            const int w = dfmi::type_width(t);
            c.values = H.bufs[HashDev::EvalOut + bi++].reserve(t == DFMI_TYPE_BOOLEAN ? (size_t)(rows + 63) / 64 * 8 : (size_t)rows * std::max(w, 1));
        }
        c.validity = (uint8_t*)H.bufs[HashDev::EvalOut + bi++].reserve((size_t)(rows + 63) / 64 * 8);
    }
    dfmi_error e{};
    if (dfmi_filter_project(ctx, pred, progs.data(), no, in, outs.data(), flags, &e) != DFMI_OK) {
        st->failed = true;
        st->failure = e;
        throw Fail{e.code, e.message};
    }
    cols.assign(no, dfmi::gb::Col{});
    for (int o = 0; o < no; ++o) {
        const dfmi_out_column& c = outs[o];
        dfmi::gb::Col& d = cols[o];
        d.type = progs[o]->type;
        d.width = d.type == DFMI_TYPE_UTF8 || d.type == DFMI_TYPE_BOOLEAN ? 0 : dfmi::type_width(d.type);
        if (c.passthrough_column >= 0) {
            const dfmi_column& src = in->columns[c.passthrough_column];
            d.values = src.values;
            d.offsets = src.offsets;
            d.validity = src.null_count > 0 ? src.validity : nullptr;
        } else {
            d.values = d.type == DFMI_TYPE_UTF8 ? (const void*)c.data : c.values;
            d.offsets = c.offsets;
            d.validity = c.null_count > 0 ? c.validity : nullptr;
        }
    }
    return outs[0].length;
}

// Key encoding for the host merge's hash index.
void encode_part(std::string& e, const KeyPart& k) {
    e.push_back(k.null ? 1 : 0);
    if (k.null) return;
    e.append((const char*)&k.ord, sizeof k.ord);
    const uint32_t l = (uint32_t)k.s.size();
    e.append((const char*)&l, 4);
    e.append(k.s);
}

// Rows `rows` (all m rows when null) of the evaluated columns merged into the
// state's groups on the host, with the kernels' per-row rules.
void host_merge_rows(dfmi_context* ctx, dfmi_agg_state* st, const std::vector<dfmi::gb::Col>& cols, int64_t m,
                     const std::vector<int32_t>* rows) {
    const size_t nk = st->keys.size(), n = st->aggs.size(), no = nk + n;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<std::vector<uint8_t>> hv(no), hb(no);
    std::vector<std::vector<int32_t>> ho(no);
    for (size_t o = 0; o < no; ++o) {
        const dfmi::gb::Col& c = cols[o];
        if (c.type == DFMI_TYPE_UTF8) {
            ho[o].resize((size_t)m + 1);
            HIP_TRY(hipMemcpy(ho[o].data(), c.offsets, ho[o].size() * 4, hipMemcpyDeviceToHost));
            const int32_t b0 = ho[o][0], b1 = ho[o][m];
            for (int32_t& x : ho[o]) x -= b0;  // (a sliced column's offsets need not start at 0)
            hv[o].resize((size_t)std::max(b1 - b0, 1));
            if (b1 > b0) HIP_TRY(hipMemcpy(hv[o].data(), (const uint8_t*)c.values + b0, (size_t)(b1 - b0),
                                           hipMemcpyDeviceToHost));
        } else {
            const size_t vb = c.type == DFMI_TYPE_BOOLEAN ? (size_t)(m + 7) / 8 : (size_t)m * c.width;
            hv[o].resize(std::max<size_t>(vb, 1));
            if (vb) HIP_TRY(hipMemcpy(hv[o].data(), c.values, vb, hipMemcpyDeviceToHost));
        }
        if (c.validity && m) {
            hb[o].resize((size_t)(m + 7) / 8);
            HIP_TRY(hipMemcpy(hb[o].data(), c.validity, hb[o].size(), hipMemcpyDeviceToHost));
        }
    }
    auto valid = [&](size_t o, int64_t i) { return hb[o].empty() || ((hb[o][i >> 3] >> (i & 7)) & 1); };
    std::vector<GroupState*> touched;
    std::string enc;
    const int64_t cnt = rows ? (int64_t)rows->size() : m;
    for (int64_t x = 0; x < cnt; ++x) {
        const int64_t i = rows ? (int64_t)(*rows)[x] : x;
        HKey hk;
        hk.p.resize(nk);
        enc.clear();
        for (size_t p = 0; p < nk; ++p) {
            KeyPart& k = hk.p[p];
            const int kt = cols[p].type;
            if (!valid(p, i)) {
                k.null = true;
            } else if (kt == DFMI_TYPE_UTF8) {
                k.s.assign((const char*)hv[p].data() + ho[p][i], (size_t)(ho[p][i + 1] - ho[p][i]));
            } else if (kt == DFMI_TYPE_BOOLEAN) {
                k = fixed_part(kt, (hv[p][i >> 3] >> (i & 7)) & 1);
            } else {
                uint64_t raw = 0;
                memcpy(&raw, hv[p].data() + (size_t)i * cols[p].width, cols[p].width);
                k = fixed_part(kt, is_signed_type(kt) ? (uint64_t)(int64_t)narrow_int(raw, kt) : narrow_int(raw, kt));
            }
            encode_part(enc, k);
        }
        GroupState* entry;
        auto ix = st->index.find(enc);
        if (ix != st->index.end()) {
            entry = ix->second;
        } else {  // first row of this key since the last reset / drain of the index
            entry = &group_entry(st->groups, std::move(hk), n);
            st->index.emplace(enc, entry);
        }
        GroupState& g = *entry;
        if (g[n].flags == 0) {  // first touch in this call: normalise it at the end
            g[n].flags = 1;
            touched.push_back(entry);
        }
        ++g[n].count;  // the group's selected rows
        for (size_t j = 0; j < n; ++j)
            if (valid(nk + j, i)) {
                host_accumulate(g[j], acc_fn(*st->aggs[j]), cols[nk + j].type, hv[nk + j].data(), i);
                if (is_utf8_extreme(*st->aggs[j])) {  // the same comparator as the device's candidate pass
                    if (g.str.size() < n) g.str.resize(n);
                    str_offer(g.str[j], st->aggs[j]->fn == DFMI_AGG_MIN, hv[nk + j].data() + ho[nk + j][i],
                              (size_t)(ho[nk + j][i + 1] - ho[nk + j][i]));
                }
            }
    }
    for (GroupState* e : touched) {  // only the entries this call touched
        for (Partial& q : *e) normalize(q);
        (*e)[n].flags = 0;
    }
}

// Bucketed accumulation (groupby.h): worth it when the batch has many rows per
// group -- the per-bucket sums then replace ~(2 + 3 per float SUM) scattered
// record atomics per row by LDS atomics, and each (bucket, split) block adds
// a group's moved words once. Needs the bucket's records in the LDS left
// beside the bucket starts (groupby.h kBucketRecordLds) and at most
// kBucketMax buckets. DFMI_DIAG=1 DFMI_GROUP_BUCKETS=0 / 1
// forces the choice (tests run small batches through both).

struct BucketShape {
    uint32_t gpb = 0;  // a power of two: 1 << gshift
    int gshift = 0;
    int nbuckets = 0, splits = 0;
};

// Records per bucket: as many as fit the LDS a block keeps beside its bucket
// starts with two blocks per CU (kBucketRecordLds); when that needs more than
// kBucketMax buckets, as many as fit one block per CU (kBucketRecordLdsBig,
// 160 KiB per workgroup on gfx950).
BucketShape bucket_shape(const HashDev& H, uint64_t ng) {
    BucketShape b;
    if (!ng) return b;
    for (int budget : {dfmi::gb::kBucketRecordLds, dfmi::gb::kBucketRecordLdsBig}) {
        const size_t fit = (size_t)budget / ((size_t)H.words * 8);
        if (!fit) continue;
        b.gshift = 0;
        while ((2ull << b.gshift) <= fit) ++b.gshift;
        b.gpb = 1u << b.gshift;
        b.nbuckets = (int)((ng + b.gpb - 1) / b.gpb);
        if (b.nbuckets <= dfmi::gb::kBucketMax) break;
    }
    b.splits = std::max(1, std::min(1024, 2048 / std::max(1, b.nbuckets)));
    return b;
}

bool use_buckets(const dfmi_agg_state* st, const HashDev& H, int64_t m, uint64_t ng, const AggDiag& diag) {
    const BucketShape b = bucket_shape(H, ng);
    if (!b.gpb || b.nbuckets > dfmi::gb::kBucketMax || st->aggs.size() > 32) return false;
    if (diag.buckets) return atoi(diag.buckets) != 0;
    // the partitioned copy of the batch (group id, NULL mask, one 8-byte word
    // per argument) stays within 16 GiB of the 288 GB
    if ((uint64_t)m * (12 + 8 * st->aggs.size()) > (16ull << 30)) return false;
    // ~4 record atomics per row against each block adding a touched group's
    // ~10 moved words once: many rows per group and split
    return (uint64_t)m >= 4ull * ng * (uint64_t)b.splits && m >= (1 << 20);
}

std::atomic<long> g_bucketed_batches{0};  // diagnostics: dfmi_internal_group_bucketed_batches
std::atomic<long> g_normalize_trips{0};   // diagnostics: dfmi_internal_group_normalize_trips
std::atomic<long> g_strided_launches{0};  // diagnostics: dfmi_internal_group_strided_launches

void accumulate_bucketed(dfmi_context* ctx, dfmi_agg_state* st, HashDev& H, const std::vector<dfmi::gb::Col>& cols,
                         int64_t m, uint64_t ng, uint32_t epoch, int grid) {
    g_bucketed_batches.fetch_add(1);
    const size_t nk = st->keys.size(), n = st->aggs.size();
    const BucketShape sh = bucket_shape(H, ng);
    const size_t nbh = (size_t)sh.nbuckets * dfmi::gb::kBucketBlocks;
    dfmi::gb::RankArgs ra{};
    for (size_t p = 0; p < nk; ++p) ra.k[p] = cols[p];
    ra.nkeys = (int)nk;
    ra.epoch = epoch;
    ra.m = m;
    ra.t = H.t;
    ra.arena = H.arena.as<uint8_t>();
    ra.arena_cap = H.arena_cap;
    ra.sidx = H.sidx.as<int32_t>();
    ra.hdr = H.dhdr();
    ra.coll_rows = H.coll.as<int32_t>();
    ra.rg = (unsigned*)H.bufs[HashDev::BucketRowGroup].reserve((size_t)m * 4);
    ra.gshift = sh.gshift;
    ra.nbuckets = sh.nbuckets;
    ra.bh = (unsigned*)H.bufs[HashDev::BucketHist].reserve(nbh * 4);
    dfmi::gb::ScatterArgs sa{};
    sa.m = m;
    sa.rg = ra.rg;
    sa.gshift = sh.gshift;
    sa.nbuckets = sh.nbuckets;
    sa.base = ra.bh;
    sa.tot = (const unsigned*)H.bufs[HashDev::BucketTotals].reserve((size_t)sh.nbuckets * 4);
    sa.naggs = (int)n;
    dfmi::gb::BucketArgs ba{};
    bool nullable = false;
    int npay = 0;
    for (size_t j = 0; j < n; ++j) {
        const dfmi::gb::Col& c = cols[nk + j];
        sa.arg[j] = c;
        nullable = nullable || c.validity;
        ba.a[j].c = c;
        ba.a[j].fn = acc_fn(*st->aggs[j]);
        ba.a[j].off = H.off[j];
        ba.pcol[j] = -1;
        const bool needs = st->aggs[j]->fn != DFMI_AGG_COUNT && c.type != DFMI_TYPE_UTF8 && c.type != DFMI_TYPE_BOOLEAN;
        if (!needs) continue;
        for (int q = 0; q < npay && ba.pcol[j] < 0; ++q)  // one payload column per distinct argument column
            if (sa.pay[q].values == c.values && sa.pay[q].type == c.type) ba.pcol[j] = q;
        if (ba.pcol[j] < 0) {
            sa.pay[npay] = c;
            ba.pcol[j] = npay++;
        }
    }
    sa.npay = npay;
    sa.pg = (unsigned*)H.bufs[HashDev::BucketPartGroup].reserve((size_t)m * 4);
    sa.pn = nullable ? (unsigned*)H.bufs[HashDev::BucketPartNull].reserve((size_t)m * 4) : nullptr;
    sa.pv = (unsigned long long*)H.bufs[HashDev::BucketPartValues].reserve((size_t)std::max(npay, 1) * (size_t)m * 8);
    ba.m = m;
    ba.tot = sa.tot;
    ba.gpb = sh.gpb;
    ba.nbuckets = sh.nbuckets;
    ba.splits = sh.splits;
    ba.ngroups = ng;
    ba.pg = sa.pg;
    ba.pn = sa.pn;
    ba.pv = sa.pv;
    ba.naggs = (int)n;
    ba.words = H.words;
    ba.acc = H.records();
    ba.pattern = H.pattern.as<unsigned long long>();
    HIP_TRY(dfmi::gb::launch_buckets(ra, sa, ba, grid, ctx->stream));
}

}  // namespace

long bucketed_batches() { return g_bucketed_batches.load(); }
long normalize_trips() { return g_normalize_trips.load(std::memory_order_relaxed); }
long strided_launches() { return g_strided_launches.load(std::memory_order_relaxed); }

// Diagnostics (dfmi_internal_group_records): the device records of groups
// [g0, g0 + ng) copied out as they stand -- nothing normalised, the table left
// as it is. info: the record's words, the groups the table holds, the float
// SUMs, then each one's digit offset in a record (3 + gb::kMaxAggs entries).
void read_records(dfmi_context* ctx, dfmi_agg_state* st, uint64_t g0, uint64_t ng, uint64_t* out, int64_t* info) {
    for (int i = 0; i < 3 + dfmi::gb::kMaxAggs; ++i) info[i] = 0;
    if (!st->hd) return;
    const HashDev& H = *st->hd;
    info[0] = H.words;
    info[1] = (int64_t)H.ngroups;
    info[2] = (int64_t)H.foff.size();
    for (size_t f = 0; f < H.foff.size(); ++f) info[3 + f] = H.foff[f];
    if (!out || !ng) return;
    if (g0 > H.ngroups || ng > H.ngroups - g0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "groups past the table's"};
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(out, H.records() + g0 * (uint64_t)H.words, ng * (size_t)H.words * 8, hipMemcpyDeviceToHost));
}

// A batch merged on the host, row by row (diagnostics: DFMI_DIAG=1
// DFMI_GROUP_HOST=1, the A/B of the device hash table).
void group_batch_on_host(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                         uint32_t flags) {
    std::vector<dfmi::gb::Col> cols;
    const int64_t m = eval_grouped(ctx, st, pred, in, flags, cols);
    if (m > 0) host_merge_rows(ctx, st, cols, m, nullptr);
}

// One batch through the device hash table: the fused evaluation pass, the
// claim pass (the table grown and the pass run again while a row finds no
// slot), the accumulate pass; rows whose key shares its hash with another
// key's are merged on the host.
void group_batch_hashed(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* in,
                        uint32_t flags, const AggDiag& diag) {
    std::vector<dfmi::gb::Col> cols;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t m = eval_grouped(ctx, st, pred, in, flags, cols);
    if (diag.finish_profile) HIP_TRY(hipStreamSynchronize(ctx->stream));
    accumulate_hashed(ctx, st, cols, m, diag, t0);
}

// A coalesced call through the device hash table: the fused Selection +
// Projection pass over [keys..., arguments...] as ONE launch
// (filter_project_batches_staged) into per-batch segments of the state's
// EvalOut buffers -- batch b's outputs at the worst-case row offset: the rows
// before b, each batch rounded up to 64 -- then the segments packed dense
// (k_group_concat; a pass-through output's source is the batch's own column)
// and the table's passes run once over the call's selected rows.
void group_batches_hashed(dfmi_context* ctx, dfmi_agg_state* st, const dfmi_program* pred, const dfmi_batch* ins,
                          int32_t nb_all, uint32_t flags, const AggDiag& diag, int32_t* failed) {
    HashDev& H = hashdev(ctx, st);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nk = st->keys.size(), n = st->aggs.size();
    const int no = (int)(nk + n);
    // (dfmi_aggregate_batch skips a batch without rows: so does the call)
    std::vector<dfmi_batch> live;
    std::vector<int32_t> index;
    for (int32_t b = 0; b < nb_all; ++b)
        if (ins[b].num_rows > 0) {
            live.push_back(ins[b]);
            index.push_back(b);
        }
    const int32_t nb = (int32_t)live.size();
    if (nb == 0) return;
    if (nb > dfmi::gb::kConcatMaxBatches) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "too many batches in one hashed call"};
    std::vector<const dfmi_program*> progs(no);
    for (size_t p = 0; p < nk; ++p) progs[p] = &st->keys[p];
    for (size_t j = 0; j < n; ++j) progs[nk + j] = &st->aggs[j]->arg;
    std::vector<int64_t> seg(nb + 1, 0);
    for (int32_t b = 0; b < nb; ++b) seg[b + 1] = seg[b] + (live[b].num_rows + 63) / 64 * 64;
    const int64_t R = seg[nb];
    std::vector<dfmi_out_column> outs((size_t)nb * no);
    memset(outs.data(), 0, outs.size() * sizeof(dfmi_out_column));
    for (int o = 0; o < no; ++o) {
        const int t = progs[o]->type;
        const int w = t == DFMI_TYPE_BOOLEAN ? 0 : std::max(dfmi::type_width(t), 1);
        uint8_t* vals = (uint8_t*)H.bufs[HashDev::EvalOut + 2 * o].reserve(w ? (size_t)R * w : (size_t)R / 8);
        uint8_t* valid = (uint8_t*)H.bufs[HashDev::EvalOut + 2 * o + 1].reserve((size_t)R / 8);
        for (int32_t b = 0; b < nb; ++b) {
            dfmi_out_column& c = outs[(size_t)b * no + o];
            c.values = vals + (w ? (size_t)seg[b] * w : (size_t)seg[b] / 8);
            c.validity = valid + (size_t)seg[b] / 8;
        }
    }
    // no predicate and every key and argument a bare column: nothing to
    // evaluate -- the first batch's pass raises what the plan raises (a
    // static error) and names the pass-through columns, the same for every batch
    bool bare = !pred;
    for (const dfmi_program* p : progs) bare = bare && p->ir[p->root].kind == IR_COL;
    dfmi_error e{};
    int32_t fb = -1;
    if (filter_project_batches_staged(ctx, pred, progs.data(), no, live.data(), bare ? 1 : nb, outs.data(), flags, &fb, &e,
                                      nullptr) != DFMI_OK) {
        st->failed = true;
        st->failure = e;
        if (fb >= 0) *failed = index[fb];
        throw Fail{e.code, e.message};
    }
    for (int32_t b = 1; bare && b < nb; ++b)
        for (int o = 0; o < no; ++o) {
            dfmi_out_column& c = outs[(size_t)b * no + o];
            c.passthrough_column = outs[o].passthrough_column;
            if (c.passthrough_column < 0) throw Fail{DFMI_ERR_DEVICE, "GROUP BY: a bare column that is not passed through"};
            if (!live[b].columns[c.passthrough_column].values)
                throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values pointer is NULL"};
            c.length = live[b].num_rows;
        }
    if (diag.finish_profile) HIP_TRY(hipStreamSynchronize(ctx->stream));
    // ---- the per-batch segments packed dense
    std::vector<long long> prefix(nb + 1, 0);
    for (int32_t b = 0; b < nb; ++b) prefix[b + 1] = prefix[b] + outs[(size_t)b * no].length;
    const int64_t m = prefix[nb];
    std::vector<dfmi::gb::Col> cols(no, dfmi::gb::Col{});
    if (m > 0) {
        std::vector<unsigned long long> srcs;
        std::vector<dfmi::gb::ConcatJob> jobs;
        for (int o = 0; o < no; ++o) {
            const int t = progs[o]->type;
            dfmi::gb::Col& d = cols[o];
            d.type = t;
            d.width = t == DFMI_TYPE_BOOLEAN ? 0 : dfmi::type_width(t);
            std::vector<unsigned long long> vsrc(nb), nsrc(nb);
            bool any_nulls = false;
            for (int32_t b = 0; b < nb; ++b) {
                const dfmi_out_column& c = outs[(size_t)b * no + o];
                if (c.passthrough_column >= 0) {
                    const dfmi_column& src = live[b].columns[c.passthrough_column];
                    vsrc[b] = (unsigned long long)src.values;
                    nsrc[b] = src.validity && src.null_count > 0 ? (unsigned long long)src.validity : 0;
                } else {
                    vsrc[b] = (unsigned long long)c.values;
                    nsrc[b] = c.null_count > 0 ? (unsigned long long)c.validity : 0;
                }
                any_nulls = any_nulls || nsrc[b];
            }
            void* dv = H.bufs[HashDev::PackOut + 2 * o].reserve(d.width ? (size_t)m * d.width : (size_t)(m + 63) / 64 * 8);
            d.values = dv;
            jobs.push_back(dfmi::gb::ConcatJob{dv, d.width, 0});
            srcs.insert(srcs.end(), vsrc.begin(), vsrc.end());
            if (any_nulls) {  // (a column with no nulls in any batch: no validity at all)
                void* dn = H.bufs[HashDev::PackOut + 2 * o + 1].reserve((size_t)(m + 63) / 64 * 8);
                d.validity = (const uint8_t*)dn;
                jobs.push_back(dfmi::gb::ConcatJob{dn, 0, 0});
                srcs.insert(srcs.end(), nsrc.begin(), nsrc.end());
            }
        }
        // the pack kernel's table: [sources | jobs | prefix]
        const size_t sb = srcs.size() * 8, jb = jobs.size() * sizeof(dfmi::gb::ConcatJob), pb = prefix.size() * 8;
        uint8_t* tab = (uint8_t*)H.bufs[HashDev::PackTable].reserve(sb + jb + pb);
        std::vector<uint8_t> htab(sb + jb + pb);
        memcpy(htab.data(), srcs.data(), sb);
        memcpy(htab.data() + sb, jobs.data(), jb);
        memcpy(htab.data() + sb + jb, prefix.data(), pb);
        HIP_TRY(hipMemcpyAsync(tab, htab.data(), htab.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // (htab is pageable: it must not go before the copy has read it)
        HIP_TRY(dfmi::gb::launch_concat((const unsigned long long*)tab, (const dfmi::gb::ConcatJob*)(tab + sb),
                                        (int)jobs.size(), (const long long*)(tab + sb + jb), nb, m, group_grid(diag),
                                        ctx->stream));
        if (diag.finish_profile) HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    accumulate_hashed(ctx, st, cols, m, diag, t0);
}

// The m evaluated rows of `cols` (keys, then arguments: one batch's, or a
// coalesced call's packed segments) through the table: claim with growth and
// rerun, record and arena growth, normalisation, accumulate, the collision list.
void accumulate_hashed(dfmi_context* ctx, dfmi_agg_state* st, const std::vector<dfmi::gb::Col>& evaluated, int64_t m,
                       const AggDiag& diag, std::chrono::steady_clock::time_point t0) {
    HashDev& H = hashdev(ctx, st);
    const bool prof = diag.finish_profile;
    const auto t1 = std::chrono::steady_clock::now();
    if (m <= 0) return;
    if (m > 0x7fffffffll) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "GROUP BY batch of 2^31 selected rows or more"};
    const size_t nk = st->keys.size(), n = st->aggs.size();
    hipStream_t stream = ctx->stream;
    const int grid = group_grid(diag);
    // a Boolean MIN / MAX is an integer extreme over 0 / 1: its bitmap expanded to a
    // UInt8 column, which every pass below (and the host merge) takes as it is
    std::vector<dfmi::gb::Col> cols = evaluated;
    for (size_t j = 0; j < n; ++j) {
        dfmi::gb::Col& c = cols[nk + j];
        if (c.type != DFMI_TYPE_BOOLEAN || st->aggs[j]->fn == DFMI_AGG_COUNT) continue;
        uint8_t* u8 = (uint8_t*)H.bufs[HashDev::BoolArg + j].reserve((size_t)(m + 7) / 8 * 8);
        HIP_TRY(dfmi::gb::launch_bits_to_u8((const uint8_t*)c.values, u8, m, grid, stream));
        c.type = DFMI_TYPE_UINT8;
        c.width = 1;
        c.values = u8;
    }
    if (H.rows_cap < m) {
        H.rows_cap = 0;
        const int64_t want = m + m / 4;
        H.sidx.alloc((size_t)want * 4);
        H.coll.alloc((size_t)want * 4);
        H.rows_cap = want;
    }
    uint64_t hash_mask = ~0ull;
    if (diag.hash_bits)  // diagnostics: a hash of so few bits that many keys share one (the host merge path)
        hash_mask = (1ull << std::max(1, std::min(63, atoi(diag.hash_bits)))) - 1;
    dfmi::gb::ClaimArgs ca{};
    for (size_t p = 0; p < nk; ++p) ca.k[p] = cols[p];
    ca.nkeys = (int)nk;
    ca.epoch = ++H.epoch;
    ca.m = m;
    ca.hash_mask = hash_mask;
    ca.hdr = H.dhdr();
    ca.sidx = H.sidx.as<int32_t>();
    for (int attempt = 0;; ++attempt) {
        ca.t = H.t;
        ca.limit = H.cap / 2;
        HIP_TRY(hipMemsetAsync(&H.dhdr()->overflow, 0, 8, stream));
        HIP_TRY(dfmi::gb::launch_claim(ca, grid, stream));
        read_hdr(ctx, H);
        if (!H.hh.p->overflow) break;
        if (H.cap >= (1ull << 31) || attempt > 16)
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "GROUP BY: more than 2^30 groups on one device"};
        grow_table(ctx, H, grid);
    }
    const uint64_t ng = H.hh.p->ngroups, aend = H.hh.p->arena_end;
    const auto t2 = std::chrono::steady_clock::now();
    if (ng > H.acc_cap) {
        uint64_t want = H.acc_cap;
        while (want < ng) want *= 2;
        H.acc.regrow(ctx->stream, H.acc_cap * (size_t)H.words * 8, want * (size_t)H.words * 8);
        HIP_TRY(dfmi::gb::launch_init(H.records(), H.pattern.as<unsigned long long>(), H.words, H.acc_cap, want, grid,
                                      stream));
        H.acc_cap = want;
    }
    if (aend > H.arena_cap) {
        uint64_t want = H.arena_cap;
        while (want < aend) want *= 2;
        H.arena.regrow(ctx->stream, H.arena_cap, want);
        H.arena_cap = want;
    }
    // exact-sum digits absorb 2^31 rows between carry normalisations
    if (!H.foff.empty() && H.rows_since_norm + (uint64_t)m > group_norm_rows(diag)) {
        g_normalize_trips.fetch_add(1, std::memory_order_relaxed);
        HIP_TRY(dfmi::gb::launch_normalize(H.records(), H.words, H.foff.data(), (int)H.foff.size(), H.ngroups, grid,
                                           stream));
        H.rows_since_norm = 0;
    }
    HIP_TRY(hipMemsetAsync(&H.dhdr()->collided, 0, 8, stream));
    // (a state with Utf8 MIN / MAX aggregates keeps the rows' group ids for the string passes)
    unsigned* rg = st->sx ? (unsigned*)H.bufs[HashDev::BucketRowGroup].reserve((size_t)m * 4) : nullptr;
    if (use_buckets(st, H, m, ng, diag)) {
        accumulate_bucketed(ctx, st, H, cols, m, ng, ca.epoch, grid);
    } else {
        dfmi::gb::AccArgs aa{};
        for (size_t p = 0; p < nk; ++p) aa.k[p] = cols[p];
        aa.nkeys = (int)nk;
        aa.epoch = ca.epoch;
        aa.m = m;
        aa.t = H.t;
        aa.arena = H.arena.as<uint8_t>();
        aa.arena_cap = H.arena_cap;
        aa.sidx = H.sidx.as<int32_t>();
        for (size_t j = 0; j < n; ++j) {
            aa.a[j].c = cols[nk + j];
            aa.a[j].fn = acc_fn(*st->aggs[j]);
            aa.a[j].off = H.off[j];
        }
        aa.naggs = (int)n;
        aa.words = H.words;
        aa.acc = H.records();
        aa.hdr = H.dhdr();
        aa.coll_rows = H.coll.as<int32_t>();
        aa.rg = rg;
        HIP_TRY(dfmi::gb::launch_accumulate(aa, grid, stream));
    }
    // Utf8 MIN / MAX: the strings of the rows added on the device (the listed rows' go with the host merge below)
    // (the records have counted the batch: a failure of the string passes fails the query)
    H.ngroups = ng;
    try {
        strext_batch(ctx, st, cols.data() + nk, rg, m, ng, diag);
    } catch (const Fail& f) {
        st->failed = true;
        set_err(&st->failure, f.code, f.msg);
        throw;
    }
    read_hdr(ctx, H);
    if (prof) {
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[dfmi add] %lld rows, %llu groups: eval %.1f us, claim %.1f us, accumulate %.1f us\n",
                (long long)m, (unsigned long long)ng, us(t0, t1), us(t1, t2), us(t2, std::chrono::steady_clock::now()));
    }
    H.ngroups = ng;
    H.rows_since_norm += (uint64_t)m;
    const uint64_t nc = H.hh.p->collided;
    if (nc) {  // rows whose key shares its 63-bit hash with another group's key
        std::vector<int32_t> rows((size_t)nc);
        HIP_TRY(hipMemcpy(rows.data(), H.coll.as<int32_t>(), (size_t)nc * 4, hipMemcpyDeviceToHost));
        std::sort(rows.begin(), rows.end());
        host_merge_rows(ctx, st, cols, m, &rows);
    }
}

namespace {

// fn(i0, i1) over [0, n) in contiguous ranges of at least `grain`, on up to
// DFMI_HOST_THREADS (default min(cores, 8)) threads.
template <typename F>
void parallel_ranges(uint64_t n, uint64_t grain, const F& fn) {
    int hw = (int)std::thread::hardware_concurrency();
    if (const char* e = getenv("DFMI_HOST_THREADS")) hw = atoi(e);
    const uint64_t ways = std::min<uint64_t>((uint64_t)std::max(1, std::min(hw, 8)), std::max<uint64_t>(1, n / grain));
    if (ways <= 1) {
        fn((uint64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    const uint64_t piece = (n + ways - 1) / ways;
    for (uint64_t w = 1; w < ways; ++w) th.emplace_back([&, w] { fn(std::min(n, w * piece), std::min(n, (w + 1) * piece)); });
    fn(0, std::min(n, piece));
    for (auto& t : th) t.join();
}

// Every group's record finished on the device (k_group_round) into the
// DrainRounded buffer: word 0 and four words per aggregate.
const unsigned long long* round_records(dfmi_context* ctx, const dfmi_agg_state* st, HashDev& H, int grid) {
    const size_t n = st->aggs.size();
    dfmi::gb::RoundArgs ra{};
    ra.acc = H.records();
    ra.words = H.words;
    ra.naggs = (int)n;
    for (size_t j = 0; j < n; ++j) {
        ra.off[j] = H.off[j];
        const int t = st->aggs[j]->arg.type;
        const int fn = st->aggs[j]->fn;
        ra.kind[j] = acc_fn(*st->aggs[j]) == DFMI_AGG_SUM && is_float_type(t)
                         ? (t == DFMI_TYPE_FLOAT32 ? 2 : 1) + (fn == DFMI_AGG_AVG ? 2 : 0)
                         : 0;
    }
    ra.ngroups = H.ngroups;
    ra.out = (unsigned long long*)H.bufs[HashDev::DrainRounded].reserve(H.ngroups * (1 + 4 * n) * 8);
    HIP_TRY(dfmi::gb::launch_round(ra, grid, ctx->stream));
    return ra.out;
}

// The groups the device hash table holds, copied out as flat arrays by group
// id (keys compacted on the device: k_group_compact), and the table emptied
// (the next batch starts a new one of the same size) -- or, `rounded` (a
// finish), every record finished on the device first (k_group_round: the
// compact records without their exact-sum digits cross PCIe) and the table
// kept as it is, so that more batches can still merge into it.
void read_table(dfmi_context* ctx, dfmi_agg_state* st, FlatGroups& f, const AggDiag& diag, bool rounded = false) {
    HashDev& H = *st->hd;
    const size_t nk = st->keys.size(), n = st->aggs.size();
    const uint64_t ng = H.ngroups;
    f.rounded = rounded;
    f.ng = ng;
    f.nk = nk;
    f.words = H.words;
    f.off = H.off;
    const unsigned long long* src = H.records();
    if (rounded) {
        for (size_t j = 0; j < n; ++j) f.off[j] = 1 + 4 * (int)j;
        f.words = 1 + 4 * (int)n;
        src = round_records(ctx, st, H, group_grid(diag));
    }
    unsigned* dnull = (unsigned*)H.bufs[HashDev::DrainNull].reserve(ng * 4);
    unsigned long long* dkw = (unsigned long long*)H.bufs[HashDev::DrainKeyWords].reserve(ng * nk * 8);
    unsigned* dklen = (unsigned*)H.bufs[HashDev::DrainKeyLens].reserve(ng * nk * 4);
    HIP_TRY(dfmi::gb::launch_compact(H.t, (int)nk, dnull, dkw, dklen, group_grid(diag), ctx->stream));
    f.knull.resize(ng);
    f.klen.resize(ng * nk);
    f.kw.resize(ng * nk);
    f.acc.resize(ng * (size_t)f.words);
    HIP_TRY(hipMemcpyAsync(f.knull.data(), dnull, ng * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f.kw.data(), dkw, ng * nk * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f.klen.data(), dklen, ng * nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f.acc.data(), src, f.acc.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    read_hdr(ctx, H);  // (synchronises the stream)
    f.arena.resize((size_t)H.hh.p->arena_end);
    if (H.hh.p->arena_end) HIP_TRY(hipMemcpy(f.arena.data(), H.arena.as<uint8_t>(), H.hh.p->arena_end, hipMemcpyDeviceToHost));
    strext_read(ctx, st, f, ng);
    if (rounded) return;
    reset_table(ctx, H, diag);  // for the next batch
    strext_reset(ctx, st, diag);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
}

// f.order: the group ids in key order (HKey's order restated on the flat
// arrays: per part, null last; integers / floats by key_ord; Utf8 bytewise,
// a shorter prefix first).
void sort_flat(const dfmi_agg_state* st, FlatGroups& f) {
    const uint64_t ng = f.ng;
    const size_t nk = f.nk;
    f.order.resize(ng);
    if (nk == 1 && st->keys[0].type != DFMI_TYPE_UTF8) {  // one fixed-width part: sort on (null, ord) values
        // LSD radix sort (16-bit digits) of the order values mapped onto
        // unsigned 64 bits (signed integers offset by 2^63); the null group last
        const int kt = st->keys[0].type;
        const bool sgn = is_signed_type(kt);
        std::vector<uint64_t> kv, kv2;
        std::vector<uint32_t> id, id2;
        kv.reserve(ng);
        id.reserve(ng);
        int64_t null_g = -1;
        for (uint64_t g = 0; g < ng; ++g) {
            if (f.knull[g] & 1) {
                null_g = (int64_t)g;
                continue;
            }
            const __int128 o = key_ord(kt, f.kw[g]);
            kv.push_back(sgn ? (uint64_t)(int64_t)o ^ (1ull << 63) : (uint64_t)o);
            id.push_back((uint32_t)g);
        }
        const size_t m = kv.size();
        if (m < 1024) {
            std::vector<std::pair<uint64_t, uint32_t>> ko(m);
            for (size_t i = 0; i < m; ++i) ko[i] = {kv[i], id[i]};
            std::sort(ko.begin(), ko.end());
            for (size_t i = 0; i < m; ++i) f.order[i] = ko[i].second;
        } else {
            // LSD radix sort, digits of D bits (8 below 2^18 groups: the counts stay in L1; 16 above);
            // a digit every key shares moves nothing and is skipped (one histogram pass finds them all)
            const int D = m < (1u << 18) ? 8 : 16, P = 64 / D;
            const size_t R = (size_t)1 << D;
            kv2.resize(m);
            id2.resize(m);
            std::vector<uint32_t> cnt(R * P, 0);
            for (size_t i = 0; i < m; ++i)
                for (int p = 0; p < P; ++p) ++cnt[(size_t)p * R + ((kv[i] >> (D * p)) & (R - 1))];
            for (int p = 0; p < P; ++p) {
                uint32_t* c = &cnt[(size_t)p * R];
                const int sh = D * p;
                if (c[(kv[0] >> sh) & (R - 1)] == m) continue;  // one digit value: this pass moves nothing
                uint32_t sum = 0;
                for (size_t d = 0; d < R; ++d) {
                    const uint32_t t = c[d];
                    c[d] = sum;
                    sum += t;
                }
                for (size_t i = 0; i < m; ++i) {
                    const uint32_t d = c[(kv[i] >> sh) & (R - 1)]++;
                    kv2[d] = kv[i];
                    id2[d] = id[i];
                }
                kv.swap(kv2);
                id.swap(id2);
            }
            std::copy(id.begin(), id.end(), f.order.begin());
        }
        if (null_g >= 0) f.order[m] = (uint32_t)null_g;
        return;
    }
    for (uint64_t g = 0; g < ng; ++g) f.order[g] = (uint32_t)g;
    std::vector<int> kt(nk);
    for (size_t p = 0; p < nk; ++p) kt[p] = st->keys[p].type;
    auto less = [&](uint32_t a, uint32_t b) {
        for (size_t p = 0; p < nk; ++p) {
            const bool na = (f.knull[a] >> p) & 1, nb = (f.knull[b] >> p) & 1;
            if (na != nb) return !na;
            if (na) continue;
            const uint64_t wa = f.kw[a * nk + p], wb = f.kw[b * nk + p];
            if (kt[p] == DFMI_TYPE_UTF8) {
                const unsigned la = f.klen[a * nk + p], lb = f.klen[b * nk + p];
                const int c = memcmp(f.arena.data() + wa, f.arena.data() + wb, std::min(la, lb));
                if (c) return c < 0;
                if (la != lb) return la < lb;
            } else if (wa != wb) {
                return key_ord(kt[p], wa) < key_ord(kt[p], wb);
            }
        }
        return false;
    };
    if (ng < 256) {
        std::sort(f.order.begin(), f.order.end(), less);
        return;
    }
    // Composite words per group, compared lexicographically: per part a null
    // flag (the null last) and a value -- a fixed-width part its order value,
    // a Utf8 part its first 8 bytes big-endian, zero-padded. LSD radix over the
    // words (8-bit digits, a digit every group shares skipped), then the runs
    // the prefixes cannot order re-sorted with the full comparator.
    const size_t W = 2 * nk;
    std::vector<uint64_t> cw(ng * W);
    bool any_utf8 = false;
    for (uint64_t g = 0; g < ng; ++g)
        for (size_t p = 0; p < nk; ++p) {
            const bool null = (f.knull[g] >> p) & 1;
            uint64_t v = 0;
            if (!null) {
                const uint64_t w = f.kw[g * nk + p];
                if (kt[p] == DFMI_TYPE_UTF8) {
                    any_utf8 = true;
                    const unsigned len = f.klen[g * nk + p];
                    const uint8_t* c = f.arena.data() + w;
                    for (unsigned q = 0; q < 8; ++q) v = (v << 8) | (q < len ? c[q] : 0u);
                } else {
                    const __int128 o = key_ord(kt[p], w);
                    v = is_signed_type(kt[p]) ? (uint64_t)(int64_t)o ^ (1ull << 63) : (uint64_t)o;
                }
            }
            cw[g * W + 2 * p] = null ? 1 : 0;
            cw[g * W + 2 * p + 1] = v;
        }
    std::vector<uint32_t> tmp(ng);
    std::vector<uint32_t> cnt(256);
    for (size_t q = W; q-- > 0;) {
        const int digits = (q & 1) ? 8 : 1;
        for (int d = 0; d < digits; ++d) {
            const int sh = 8 * d;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (uint64_t i = 0; i < ng; ++i) ++cnt[(cw[(size_t)f.order[i] * W + q] >> sh) & 0xff];
            if (cnt[(cw[(size_t)f.order[0] * W + q] >> sh) & 0xff] == ng) continue;
            uint32_t sum = 0;
            for (auto& c : cnt) {
                const uint32_t t = c;
                c = sum;
                sum += t;
            }
            for (uint64_t i = 0; i < ng; ++i) tmp[cnt[(cw[(size_t)f.order[i] * W + q] >> sh) & 0xff]++] = f.order[i];
            std::copy(tmp.begin(), tmp.end(), f.order.begin());
        }
    }
    if (!any_utf8) return;
    // the word order is exact up to the first Utf8 part's prefix: groups that
    // agree on every word up to it may be out of order (the rest of that part
    // decides before any later part), so each such run is re-sorted in full
    size_t p1 = 0;
    while (kt[p1] != DFMI_TYPE_UTF8) ++p1;
    const size_t E = 2 * p1 + 2;
    auto same = [&](uint32_t a, uint32_t b) {
        return std::equal(cw.begin() + (size_t)a * W, cw.begin() + (size_t)a * W + E, cw.begin() + (size_t)b * W);
    };
    for (uint64_t i = 0; i < ng;) {
        uint64_t j = i + 1;
        while (j < ng && same(f.order[i], f.order[j])) ++j;
        if (j - i > 1) std::sort(f.order.begin() + i, f.order.begin() + j, less);
        i = j;
    }
}

// Aggregate j's partial of group record `rec` (the device record layout:
// groupby.h; word 0 the group's rows).
void rec_partial(const dfmi_agg_state* st, const FlatGroups& f, const uint64_t* rec, size_t j, Partial& q) {
    const uint64_t* w = rec + f.off[j];
    const int fn = acc_fn(*st->aggs[j]);
    q.count = rec[0] - w[0];  // the group's rows minus its NULL arguments
    if (fn == DFMI_AGG_SUM && is_float_type(st->aggs[j]->arg.type)) {
        q.flags = (w[1] & 0xffffffffull) | (q.count > w[3] ? AGGF_NONNEGZERO : 0);
        if (f.rounded) return;  // (the digits were rounded on the device: w[2])
        for (int i = 0; i < kAggLimbs; ++i) q.limbs[i] = (int64_t)w[4 + i];
        normalize(q);
    } else if (fn == DFMI_AGG_SUM) {
        q.isum = w[3];
    } else if (fn == DFMI_AGG_MIN || fn == DFMI_AGG_MAX) {
        q.key = w[2];
        q.flags = (w[3] ? AGGF_NAN : 0) | (q.count > w[3] ? AGGF_VALUE : 0);
    }
}

// The flat groups merged into st->groups (into an empty map in key order:
// each insertion O(1) at its end).
void materialize_flat(dfmi_agg_state* st, FlatGroups& f) {
    const size_t nk = f.nk, n = st->aggs.size();
    const bool fresh = st->groups.empty();
    if (fresh && f.order.size() != f.ng) sort_flat(st, f);
    for (uint64_t i = 0; i < f.ng; ++i) {
        const uint32_t g = fresh ? f.order[i] : (uint32_t)i;
        HKey hk;
        hk.p.resize(nk);
        for (size_t p = 0; p < nk; ++p) {
            KeyPart& k = hk.p[p];
            const int kt = st->keys[p].type;
            if ((f.knull[g] >> p) & 1) k.null = true;
            else if (kt == DFMI_TYPE_UTF8) k.s.assign((const char*)f.arena.data() + f.kw[g * nk + p], f.klen[g * nk + p]);
            else k = fixed_part(kt, f.kw[g * nk + p]);
        }
        const uint64_t* rec = &f.acc[(size_t)g * f.words];
        GroupState parts(n + 1);
        parts[n].count = rec[0];
        for (size_t j = 0; j < n; ++j) rec_partial(st, f, rec, j, parts[j]);
        if (st->sx) {
            parts.str.resize(n);
            for (size_t x = 0; x < st->sx->x.size(); ++x) parts.str[st->sx->x[x].agg] = strext_flat_value(f, x, g);
        }
        if (fresh) {
            st->groups.emplace_hint(st->groups.end(), std::move(hk), std::move(parts));
        } else {
            merge_group(group_entry(st->groups, std::move(hk), n), parts, st->aggs.data(), n);
        }
    }
}

std::unique_ptr<FlatGroups> take_flat(dfmi_agg_state* st) {
    std::unique_ptr<FlatGroups> f = st->spare_flat ? std::move(st->spare_flat) : std::make_unique<FlatGroups>();
    f->order.clear();
    return f;
}

}  // namespace

// An empty table of the same size (enqueued on the stream).
void reset_table(dfmi_context* ctx, HashDev& H, const AggDiag& diag) {
    HIP_TRY(hipMemsetAsync(H.t.ctl, 0, H.cap * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(H.hdr.p, 0, sizeof(dfmi::gb::Hdr), ctx->stream));
    HIP_TRY(dfmi::gb::launch_init(H.records(), H.pattern.as<unsigned long long>(), H.words, 0, H.ngroups, group_grid(diag),
                                  ctx->stream));
    H.ngroups = 0;
    H.rows_since_norm = 0;
}

// A finish's flat groups (st->flat) moved into st->groups before anything
// else merges into or reads the map (a device-finished snapshot is dropped:
// the device table still holds its groups).
void unflatten(dfmi_agg_state* st) {
    if (!st->flat) return;
    std::unique_ptr<FlatGroups> f = std::move(st->flat);
    if (!f->rounded) materialize_flat(st, *f);
    st->spare_flat = std::move(f);
}

// The groups the device hash table holds merged into st->groups, and the
// table emptied.
void drain_hashed(dfmi_context* ctx, dfmi_agg_state* st) {
    unflatten(st);
    if (!st->hd || !st->hd->ngroups) return;
    std::unique_ptr<FlatGroups> f = take_flat(st);
    read_table(ctx, st, *f, agg_diag());
    materialize_flat(st, *f);
    st->spare_flat = std::move(f);
}

// The finish of a state whose groups all sit in the device hash table (no
// window flush, no host merge: the common case): every group finished on the
// device, the results kept flat (st->flat, sorted by key) and emitted from
// there -- no per-group map node, key string, partial copy or exact-sum
// digits on the host; the table keeps the groups for later batches. (The
// caller has flushed the key window.)
bool finish_flat(dfmi_context* ctx, dfmi_agg_state* st, const AggDiag& diag) {
    if (!st->groups.empty()) return false;
    if (st->flat && !st->flat->rounded && st->hd && st->hd->ngroups) return false;  // (a batch unflattens first)
    if (!st->flat) {
        if (!st->hd || !st->hd->ngroups) return false;
        std::unique_ptr<FlatGroups> f = take_flat(st);
        const auto t0 = std::chrono::steady_clock::now();
        read_table(ctx, st, *f, diag, !diag.host_finish);
        const auto t1 = std::chrono::steady_clock::now();
        sort_flat(st, *f);
        if (diag.finish_profile)
            fprintf(stderr, "[dfmi finish] %llu groups: read_table %.1f us, sort %.1f us\n", (unsigned long long)f->ng,
                    std::chrono::duration<double, std::micro>(t1 - t0).count(),
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count());
        st->flat = std::move(f);
    }
    st->shown.reset();
    return true;
}

// The finish of one fixed-width key with many groups, ordered and emitted on
// the device (groupby.h EmitArgs): round, compact, sort values, radix sort,
// emission; only the caller's dfmi_agg_value arrays cross PCIe. Taken from
// kDeviceEmitMin groups (below, the host's sort and emission cost less than
// the launches; at 10^4 groups the device path saves 0.7 ms per finish, at
// 10^6 ~35 ms); DFMI_DIAG=1 DFMI_GROUP_DEVICE_EMIT=0 / 1 forces the choice.
// (The caller has flushed the key window.)
constexpr uint64_t kDeviceEmitMin = 2048;
static_assert(sizeof(dfmi_agg_value) == 24, "dfmi_agg_value as groupby.hip AggValue");

bool finish_device(dfmi_context* ctx, dfmi_agg_state* st, const AggDiag& diag, int64_t cap, dfmi_agg_value* keys,
                   dfmi_agg_value* values, int64_t* num_groups) {
    if (st->keys.size() != 1 || st->keys[0].type == DFMI_TYPE_UTF8 || !st->hd ||
        st->aggs.size() > (size_t)dfmi::gb::kMaxAggs)
        return false;
    if (diag.host_finish || st->sx) return false;  // (a Utf8 MIN / MAX's bytes are joined on the host)
    const char* force = diag.device_emit;
    if (force && !atoi(force)) return false;
    if (!st->groups.empty() || (st->flat && !st->flat->rounded)) return false;
    HashDev& H = *st->hd;
    const uint64_t ng = H.ngroups;
    if (!ng || (!force && ng < kDeviceEmitMin)) return false;
    *num_groups = (int64_t)ng;
    if (*num_groups > cap) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "group capacity too small"};
    if (!keys || !values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
    if (st->flat) st->spare_flat = std::move(st->flat);
    const size_t n = st->aggs.size();
    hipStream_t stream = ctx->stream;
    const int grid = group_grid(diag);
    dfmi::gb::EmitArgs ea{};
    for (size_t j = 0; j < n; ++j) {
        ea.fn[j] = st->aggs[j]->fn;
        ea.atype[j] = st->aggs[j]->arg.type;
        ea.rtype[j] = st->aggs[j]->ret_type;
    }
    ea.rec = round_records(ctx, st, H, grid);
    unsigned* dnull = (unsigned*)H.bufs[HashDev::DrainNull].reserve(ng * 4);
    unsigned long long* dkw = (unsigned long long*)H.bufs[HashDev::DrainKeyWords].reserve(ng * 8);
    unsigned* dklen = (unsigned*)H.bufs[HashDev::DrainKeyLens].reserve(ng * 4);
    HIP_TRY(dfmi::gb::launch_compact(H.t, 1, dnull, dkw, dklen, grid, stream));
    ea.knull = dnull;
    ea.kw = dkw;
    ea.ngroups = ng;
    ea.ktype = st->keys[0].type;
    ea.naggs = (int)n;
    ea.keys = H.bufs[HashDev::EmitKeys].reserve(ng * sizeof(dfmi_agg_value));
    ea.values = H.bufs[HashDev::EmitValues].reserve(ng * n * sizeof(dfmi_agg_value));
    auto* sk = (unsigned long long*)H.bufs[HashDev::EmitSortKeys].reserve(ng * 8);
    auto* sk2 = (unsigned long long*)H.bufs[HashDev::EmitSortKeys2].reserve(ng * 8);
    auto* sv = (unsigned*)H.bufs[HashDev::EmitSortVals].reserve(ng * 4);
    auto* sv2 = (unsigned*)H.bufs[HashDev::EmitSortVals2].reserve(ng * 4);
    auto* null_at = (unsigned*)H.bufs[HashDev::EmitNullAt].reserve(8);
    size_t tb = 0;
    HIP_TRY(dfmi::gb::launch_emit(ea, sk, sk2, sv, sv2, null_at, nullptr, &tb, grid, stream));
    void* tmp = H.bufs[HashDev::EmitTemp].reserve(tb);
    HIP_TRY(dfmi::gb::launch_emit(ea, sk, sk2, sv, sv2, null_at, tmp, &tb, grid, stream));
    HIP_TRY(hipMemcpyAsync(keys, ea.keys, ng * sizeof(dfmi_agg_value), hipMemcpyDeviceToHost, stream));
    if (n) HIP_TRY(hipMemcpyAsync(values, ea.values, ng * n * sizeof(dfmi_agg_value), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    st->shown.reset();
    return true;
}

void emit_flat(const dfmi_agg_state* st, const FlatGroups& f, int64_t cap, dfmi_agg_value* keys,
               dfmi_agg_value* values, int64_t* num_groups) {
    *num_groups = (int64_t)f.ng;
    if (*num_groups > cap) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "group capacity too small"};
    if (*num_groups > 0 && (!keys || !values)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
    const size_t nk = f.nk, n = st->aggs.size();
    std::vector<int> xof(n, -1);  // aggregate j's index among the Utf8 MIN / MAX aggregates
    if (st->sx)
        for (size_t x = 0; x < st->sx->x.size(); ++x) xof[st->sx->x[x].agg] = (int)x;
    auto emit_range = [&](uint64_t i0, uint64_t i1) {
        Partial q;
        for (uint64_t i = i0; i < i1; ++i) {
            const uint32_t g = f.order[i];
            const uint64_t* rec = &f.acc[(size_t)g * f.words];
            for (size_t p = 0; p < nk; ++p) {
                dfmi_agg_value& k = keys[i * nk + p];
                const int kt = st->keys[p].type;
                const bool null = (f.knull[g] >> p) & 1;
                k.type = kt;
                k.is_null = null ? 1 : 0;
                k.bits = null || kt == DFMI_TYPE_UTF8 ? 0
                                                      : (kt == DFMI_TYPE_BOOLEAN ? f.kw[g * nk + p] : narrow_int(f.kw[g * nk + p], kt));
                k.count = (int64_t)rec[0];
            }
            for (size_t j = 0; j < n; ++j) {
                q.flags = q.key = q.isum = 0;  // (rec_partial sets count and, for a float SUM, every digit)
                rec_partial(st, f, rec, j, q);
                if (f.rounded && acc_fn(*st->aggs[j]) == DFMI_AGG_SUM && is_float_type(st->aggs[j]->arg.type)) {
                    const uint64_t* w = rec + f.off[j];
                    Rounded r;
                    memcpy(&r.v, &w[2], 8);
                    r.zero = (w[1] & dfmi::gb::kRoundZero) != 0;
                    values[i * n + j] = finish_normalized(*st->aggs[j], q, &r);
                } else {
                    values[i * n + j] = finish_normalized(*st->aggs[j], q);
                    if (xof[j] >= 0 && !values[i * n + j].is_null) {  // the value's byte length
                        const dfmi::sx::Ent& e = f.sx_ent[(size_t)xof[j]][g];
                        values[i * n + j].bits = e.len == dfmi::sx::kNone ? 0 : e.len;
                    }
                }
            }
        }
    };
    parallel_ranges(f.ng, 32768, emit_range);  // (a thread's start costs more than ~10^4 groups' emission)
}

void emit_key_bytes_flat(const FlatGroups& f, int part, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                         int64_t data_capacity, int64_t* data_length) {
    const size_t nk = f.nk;
    int64_t total = 0;
    for (uint64_t g = 0; g < f.ng; ++g)
        if (!((f.knull[g] >> part) & 1)) total += f.klen[g * nk + part];
    *data_length = total;
    if (total > 0x7fffffffll) throw Fail{DFMI_ERR_CAPACITY, "Utf8 group keys of 2^31 bytes or more"};
    if (num_offsets < (int64_t)f.ng + 1 || data_capacity < total)
        throw Fail{DFMI_ERR_CAPACITY, "key offsets / bytes capacity too small"};
    if (!offsets || (total && !data)) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL argument"};
    int64_t pos = 0;
    offsets[0] = 0;
    for (uint64_t i = 0; i < f.ng; ++i) {
        const uint32_t g = f.order[i];
        if (!((f.knull[g] >> part) & 1)) {
            const unsigned len = f.klen[g * nk + part];
            if (len) memcpy(data + pos, f.arena.data() + f.kw[g * nk + part], len);
            pos += len;
        }
        offsets[i + 1] = (int32_t)pos;
    }
}

}  // namespace agg
}  // namespace dfmi

// groupby.h "Diagnostic grid cap": a kernel launch took more than one trip of its grid.
void dfmi::gb::count_strided_launch() { dfmi::agg::g_strided_launches.fetch_add(1, std::memory_order_relaxed); }
