// The host paths' layouts (host_plan.h). Host only: built without a device
// for the sanitizer driver (tests/native).
#include "host_plan.h"

#include <algorithm>
#include <cstdlib>

#include "abi_guard.h"
#include "col_layout.h"

namespace dfmi {

void check_shared_schema(const dfmi_batch* ins, int32_t nb, bool host_pointers) {
    const int ncols = ins[0].num_columns;
    for (int32_t b = 0; b < nb; ++b) {
        if (ins[b].num_columns != ncols || (ncols > 0 && !ins[b].columns))
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batches do not share a schema"};
        for (int i = 0; i < ncols; ++i) {
            const dfmi_column& c = ins[b].columns[i];
            if (c.type != ins[0].columns[i].type) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batches do not share a schema"};
            if (c.length != ins[b].num_rows) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "ragged batch"};
            if (!host_pointers) continue;
            if (c.type == DFMI_TYPE_UTF8 && !c.offsets) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "Utf8 offsets are NULL"};
            if (!c.values && col_bytes(c, c.length).values)
                throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values pointer is NULL"};
        }
    }
}

namespace host {

int64_t chunk_rows_for(int64_t n, double in_bytes_per_row) {
    int64_t r;
    if (const char* e = getenv("DFMI_HOST_CHUNK_ROWS")) {
        r = std::max<int64_t>(512, atoll(e));
    } else {
        constexpr double kTarget = 48.0 * (1 << 20);
        r = (int64_t)(kTarget / std::max(in_bytes_per_row, 1.0));
        r = std::max<int64_t>(r, 1 << 16);
        if (n <= r + r / 2) return std::max<int64_t>(n, 1);
    }
    r &= ~(int64_t)511;
    r = std::max<int64_t>(r, 512);
    return n <= r ? std::max<int64_t>(n, 1) : r;
}

std::vector<Chunk> chunks_of(int64_t n, int64_t crows) {
    std::vector<Chunk> chunks;
    for (int64_t r0 = 0; r0 < n || chunks.empty(); r0 += crows) chunks.push_back({r0, std::min(crows, n - r0)});
    return chunks;
}

Shape call_shape(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch& in) {
    Shape S;
    const int64_t n = in.num_rows;
    const int ncols = S.ncols = in.num_columns;
    const int nout = S.nout = np > 0 ? np : ncols;
    S.otype.assign(nout, 0);
    S.osrc.assign(nout, -1);
    S.passthrough.assign(nout, 0);
    S.need.assign(std::max(0, ncols), 0);
    mark_columns(pred, S.need);
    for (int o = 0; o < nout; ++o) {
        if (np > 0) {
            if (!projs[o]) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL projection"};
            S.otype[o] = projs[o]->type;
            const IrNode& root = projs[o]->ir[projs[o]->root];
            if (root.kind == IR_COL) S.osrc[o] = root.col;
            S.passthrough[o] = !pred && root.kind == IR_COL;
            if (!S.passthrough[o]) mark_columns(projs[o], S.need);
        } else {
            S.otype[o] = in.columns[o].type;
            S.osrc[o] = o;
            if (pred) S.need[o] = 1;  // FilterRelation gathers every column (filter.rs:80-111)
        }
    }
    for (int i = 0; i < ncols; ++i) {
        const dfmi_column& c = in.columns[i];
        if (c.length != n) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "ragged batch"};
        if (c.type == DFMI_TYPE_UTF8 && !c.offsets) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "Utf8 offsets are NULL"};
        const size_t values = col_bytes(c, n).values;
        if (!c.values && values) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "column values pointer is NULL"};
        if (!S.need[i]) continue;
        S.in_bpr += c.type == DFMI_TYPE_BOOLEAN ? 0.125 : type_width(c.type);
        if (c.validity) S.in_bpr += 0.125;
        if (c.type == DFMI_TYPE_UTF8) S.in_bpr += 4.0 + (n ? (double)values / n : 0);
    }
    return S;
}

InPlan plan_chunk_in(const dfmi_batch& in, const std::vector<char>& need, const Chunk& ch, PinnedFn pinned) {
    const int ncols = in.num_columns;
    InPlan P;
    P.bufs.assign((size_t)3 * std::max(ncols, 1), Buf{});
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < ncols; ++i) {
            if (!need[i]) continue;
            const dfmi_column& c = in.columns[i];
            const int64_t r0 = ch.r0, m = ch.rows;
            Buf v, b, of;
            if (c.type == DFMI_TYPE_UTF8) {
                const int32_t s0 = c.offsets[r0], s1 = c.offsets[r0 + m];
                v.src = (const uint8_t*)c.values + s0;
                v.bytes = (size_t)std::max(0, s1 - s0);
                of.src = (const uint8_t*)(c.offsets + r0);
                of.bytes = (size_t)(m + 1) * 4;
            } else {
                const size_t w = (size_t)type_width(c.type);  // (0: Boolean, a bitmap)
                v.src = (const uint8_t*)c.values + (w ? r0 * (int64_t)w : r0 / 8);
                v.bytes = w ? (size_t)m * w : (size_t)(m + 7) / 8;
            }
            if (c.validity) {  // (staged whenever the column carries one)
                b.src = c.validity + r0 / 8;
                b.bytes = (size_t)(m + 7) / 8;
            }
            Buf* dst[3] = {&v, &b, &of};
            const bool exists[3] = {true, c.validity != nullptr, c.type == DFMI_TYPE_UTF8};
            for (int k = 0; k < 3; ++k) {
                if (!exists[k]) continue;
                Buf& x = *dst[k];
                x.direct = x.bytes && pinned(x.src, x.bytes);
                if (x.direct != (pass == 1)) continue;
                // device side: >= 8 bytes (a kernel reads whole words)
                x.off = P.total;
                P.total += align256(std::max<size_t>(x.bytes + 8, 16));
                if (pass == 0) P.staged_bytes = P.total;
                P.bufs[(size_t)3 * i + k] = x;
            }
        }
    }
    return P;
}

OutRegion plan_chunk_out(const Shape& S, const std::vector<InPlan>& inplans, int64_t rows_cap) {
    OutRegion R;
    R.col.assign(S.nout, OutPlan{});
    size_t cap = 0;
    for (int o = 0; o < S.nout; ++o) {
        if (S.passthrough[o]) continue;
        const int t = S.otype[o];
        OutPlan& p = R.col[o];
        if (t == DFMI_TYPE_UTF8) {
            size_t dc = 8;
            if (S.osrc[o] >= 0)
                for (const InPlan& P : inplans) dc = std::max(dc, P.bufs[(size_t)3 * S.osrc[o]].bytes);
            p.offsets = cap;
            cap += align256((size_t)(rows_cap + 1) * 4);
            p.data = cap;
            p.data_cap = dc;
            cap += align256(dc + 8);
        } else {
            p.values = cap;
            p.values_cap = t == DFMI_TYPE_BOOLEAN ? bitmap_bytes(rows_cap) : (size_t)rows_cap * std::max(type_width(t), 1);
            cap += align256(p.values_cap + 8);
            p.validity = cap;
            cap += align256(bitmap_bytes(rows_cap) + 8);
            if (t == DFMI_TYPE_BOOLEAN) p.bm_values = R.n_bm++;
            p.bm_valid = R.n_bm++;
        }
    }
    R.bytes = std::max<size_t>(cap, 256);
    return R;
}

void hb_layout(const dfmi_program* pred, const dfmi_program* const* projs, int32_t np, const dfmi_batch* ins,
               int32_t nb, HBLayout& Lo) {
    if (!pred && np == 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "neither a predicate nor projections"};
    const int ncols = ins[0].num_columns;
    const int nout = np > 0 ? np : ncols;
    Lo.ncols = ncols;
    Lo.nout = nout;
    check_shared_schema(ins, nb, true);
    // ---- input layout: per batch and column, values / offsets / validity
    Lo.lay.assign((size_t)nb * ncols, HBLayout::In{});
    size_t in_bytes = 0;
    for (int32_t b = 0; b < nb; ++b)
        for (int i = 0; i < ncols; ++i) {
            const dfmi_column& c = ins[b].columns[i];
            const ColBytes cb = col_bytes(c, c.length);
            HBLayout::In& L = Lo.lay[(size_t)b * ncols + i];
            L.nval = cb.values;
            L.val = in_bytes;
            in_bytes += align256(L.nval);
            if (c.type == DFMI_TYPE_UTF8) {
                L.noff = cb.offsets;
                L.off = in_bytes;
                in_bytes += align256(L.noff);
            }
            if (c.null_count > 0 && cb.validity) {  // (a bitmap without nulls is not staged)
                L.nvld = cb.validity;
                L.vld = in_bytes;
                in_bytes += align256(L.nvld);
            }
        }
    // ---- output layout (worst case per batch: every row selected)
    Lo.otype.assign(nout, 0);
    for (int o = 0; o < nout; ++o) {
        if (np > 0 && !projs[o]) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "NULL projection"};
        Lo.otype[o] = np > 0 ? projs[o]->type : ins[0].columns[o].type;
    }
    auto osrc = [&](int o) -> int {  // the input column a Utf8 output gathers
        if (np == 0) return o;
        const IrNode& root = projs[o]->ir[projs[o]->root];
        return root.kind == IR_COL ? root.col : -1;
    };
    Lo.olay.assign((size_t)nb * nout, HBLayout::Out{});
    size_t out_bytes = 0;
    for (int32_t b = 0; b < nb; ++b)
        for (int o = 0; o < nout; ++o) {
            const int64_t n = ins[b].num_rows;
            HBLayout::Out& L = Lo.olay[(size_t)b * nout + o];
            const int t = Lo.otype[o];
            L.val = out_bytes;
            out_bytes += align256(t == DFMI_TYPE_BOOLEAN ? (size_t)bitmap_bytes(n)
                                                         : (t == DFMI_TYPE_UTF8 ? 0 : (size_t)n * type_width(t)));
            L.vld = out_bytes;
            out_bytes += align256(bitmap_bytes(n));
            if (t == DFMI_TYPE_UTF8) {
                L.off = out_bytes;
                out_bytes += align256((size_t)(n + 1) * 4);
                const int c = osrc(o);
                L.ndat = c >= 0 ? col_bytes(ins[b].columns[c], ins[b].columns[c].length).values : 0;
                L.dat = out_bytes;
                out_bytes += align256(std::max<size_t>(L.ndat, 1));
            }
        }
    Lo.in_bytes = in_bytes;
    Lo.out_bytes = out_bytes;
    Lo.OB = align256(std::max<size_t>(out_bytes, 256));
    Lo.H = align256((size_t)nb * 256);
    Lo.IB = align256(std::max<size_t>(in_bytes, 256));
    size_t MB = 256;  // bound on the launch's batch table + tile map (batch_table.h)
    for (int32_t b = 0; b < nb; ++b)
        MB += (size_t)(4 + 3 * ncols + 5 * nout) * 8 + (size_t)((ins[b].num_rows + 63) / 64 + 1) * 4;
    Lo.MB = align256(MB);
}

}  // namespace host
}  // namespace dfmi
