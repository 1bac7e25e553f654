// Query compiler, kernel bodies: writes the query's Selection + Projection as one
// straight-line gfx950 kernel over the hand-written skeleton
// (jit_skeleton.hip); jit_expr.cpp writes the expressions inside it, and
// jit_cache.cpp compiles it with hipRTC once per query shape. Replaces the per-row interpretation of the reference's
// compiled closures (expression.rs:29-451, filter.rs:80-111) -- and of an
// earlier device interpreter here, whose per-operator decode made the pass
// scalar-issue bound (DESIGN.md "Kernels").
//
// Shape of every generated kernel (filtered form):
//   1. load the predicate's columns for the thread's K rows (all loads first);
//   2. evaluate the predicate per row -> selection bits;
//   3. lane-masked loads of projection-only columns (only where selected);
//   4. ballot / per-(k,wave) counts, tile scan, decoupled look-back;
//   5. evaluate projections, store compacted rows; Utf8 gathers.
// Literal values and buffer addresses are kernel arguments, so one binary
// serves every instance of a query shape.
#include <algorithm>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "jit_gen.h"

extern const char dfmi_skeleton_src[];  // jit_skeleton.hip, embedded by the Makefile

namespace dfmi {
namespace jit {

const std::string& skeleton_text() {
    static const std::string s(dfmi_skeleton_src);
    return s;
}

namespace {

// --------------------------------------------------------------- kernels
// Register arrays of the given slots.
void emit_decls(std::ostream& o, const std::vector<int>& slots, const Launch& X, bool valid_words) {
    for (int s : slots) {
        const int col = X.num_cols[s];
        const int ty = X.col_type(col);
        if (ty == DFMI_TYPE_BOOLEAN)
            o << "  u64 bw" << s << "[K];\n";
        else
            o << "  " << ctype(ty) << " c" << s << "[K];\n";
        if (valid_words && X.col_nullable(col)) o << "  u64 vw" << s << "[K];\n";
    }
}

// Loads of the K rows per thread of the tile at `base` (wave-uniform): a
// branch-free form for full tiles and a guarded one for the last tile. Value
// loads of projection-only slots are lane-masked by `guard` (selected rows).
void emit_loads(std::ostream& o, const std::vector<int>& slots, const Launch& X, const std::string& base,
                const char* guard, bool valid_words) {
    if (slots.empty()) return;
    for (int full = 1; full >= 0; --full) {
        o << (full ? "  if (A.n_rows - " + base + " >= BLOCK * K) {\n" : "  } else {\n");
        for (int s : slots) {
            const int col = X.num_cols[s];
            if (X.col_type(col) == DFMI_TYPE_BOOLEAN) {
                o << "#pragma unroll\n    for (int k = 0; k < K; ++k) bw" << s
                  << "[k] = dfmi::bitmap_word((const u8*)A.col[" << s << "], (" << base
                  << " >> 6) + k * WAVES + wave, A.n_rows);\n";
            } else {
                // 64 lanes x width bytes per wave load, contiguous in row order
                std::string g = guard ? std::string(guard) : "";
                if (!full) g = g.empty() ? "(" + base + " + k * BLOCK + tid < A.n_rows)"
                                         : "(" + base + " + k * BLOCK + tid < A.n_rows) && " + g;
                const std::string ct = ctype(X.col_type(col));
                const std::string ld = (X.nt & 1) ? "__builtin_nontemporal_load(p_ + k * BLOCK)" : "p_[k * BLOCK]";
                o << "    { const " << ct << "* p_ = (const " << ct << "*)A.col[" << s << "] + " << base << " + tid;\n"
                  << "#pragma unroll\n      for (int k = 0; k < K; ++k) c" << s << "[k] = "
                  << (g.empty() ? ld + ";" : "(" + g + ") ? " + ld + " : (" + ct + ")0;") << " }\n";
            }
            if (valid_words && X.col_nullable(col)) {
                o << "#pragma unroll\n    for (int k = 0; k < K; ++k) vw" << s << "[k] = dfmi::bitmap_word(A.valid[" << s
                  << "], (" << base << " >> 6) + k * WAVES + wave, A.n_rows);\n";
            }
        }
    }
    o << "  }\n";
}

// The numeric / Boolean slots program p's columns are in, added to `out` (once each).
void add_col_slots(std::vector<int>& out, const Launch& X, int col) {
    for (size_t s = 0; s < X.num_cols.size(); ++s)
        if (X.num_cols[s] == col && std::find(out.begin(), out.end(), (int)s) == out.end()) out.push_back((int)s);
}
void add_prog_slots(std::vector<int>& out, const Launch& X, const dfmi_program* p) {
    for (const IrNode& nd : p->ir)
        if (nd.kind == IR_COL) add_col_slots(out, X, nd.col);
}

// Numeric / Boolean slots the outputs read (a sub-tile kernel's output pass
// reloads exactly these for the selected rows).
std::vector<int> output_slots(const Plan& P, const Launch& X) {
    std::vector<int> out;
    for (const OutSpec& os : P.outs) {
        if (os.kind == OutSpec::GATHER) add_col_slots(out, X, os.col);
        if (os.kind == OutSpec::EXPR) add_prog_slots(out, X, os.prog);
    }
    std::sort(out.begin(), out.end());
    return out;
}

// Declares Utf8 slot u's offset registers us<n><u> / ux<n><u> and loads them
// for the slices of the tile at `base` that `mask` names.
void emit_offs_tile(std::ostream& o, int u, const char* n, const char* base, const char* mask) {
    o << "  int us" << n << u << "[K], ux" << n << u << "[K];\n  dfmi::utf8_offs_tile<BLOCK, K>(A, " << u << ", " << base
      << ", lane, wave, " << mask << ", us" << n << u << ", ux" << n << u << ");\n";
}

// The predicate of a filtered tile: `unsigned selm` (bit k = row base + k*BLOCK
// + tid selected, mask.value(i)); Utf8 columns' offsets (us<u> / ux<u>) are
// loaded tile-wide in front of the predicate loop -- the predicate's `col =
// literal` compares and the columns in `extra_offs` (Utf8 outputs: their byte
// counts are needed before the look-back, so they share the first memory
// round trip). Returns the Utf8 slots whose offsets are in registers.
std::vector<int> emit_predicate(Gen& g, std::ostream& o, const std::vector<int>& extra_offs, bool preloaded = false) {
    const Plan& P = g.P;
    const Launch& X = g.X;
    // the loop goes to a stream of its own: what it reads from the tile-wide
    // pre-pass is only known once it is written, and goes in front of it
    std::ostringstream loop;
    std::ostream* const outer = g.out;
    g.out = &loop;
    g.tile_pre = true;
    g.pre_eq.clear();
    g.pre_ord.clear();
    loop << "  unsigned selm = 0;\n#pragma unroll\n  for (int k = 0; k < K; ++k) {\n";
    loop << "    const i64 row = base + k * BLOCK + tid;\n    const bool in = row < A.n_rows;\n";
    const Val r = g.emit(P.pred, P.pred->root, 0, "in");
    if (P.pred->type == DFMI_TYPE_BOOLEAN && !r.v.empty())
        loop << "    selm |= (unsigned)(in && (" << r.v << ")) << k;\n";  // mask.value(i)
    loop << "  }\n";
    g.tile_pre = false;
    g.out = outer;
    std::vector<int> offs_loaded;
    auto load_offs = [&](int u) {
        if (std::find(offs_loaded.begin(), offs_loaded.end(), u) != offs_loaded.end()) return;
        offs_loaded.push_back(u);
        if (!preloaded) emit_offs_tile(o, u, "", "base", "~0u");  // (else in scope already: sub-tile prefetch)
    };
    for (const auto& pe : g.pre_eq) load_offs(std::get<1>(pe));
    for (const auto& pe : g.pre_ord) load_offs(std::get<1>(pe));
    for (int u : extra_offs) load_offs(u);
    for (const auto& [arr, u, sl] : g.pre_eq) {
        o << "  bool " << arr << "[K];\n  dfmi::utf8_eq_lit_tile";
        if (X.eq_dense < 0)
            o << "_reg<BLOCK, K, " << -X.eq_dense << ">";
        else if (X.eq_dense)
            o << "_dense<BLOCK, K, " << X.eq_dense << ">";
        else
            o << "<BLOCK, K>";
        o << "(A, " << u << ", " << sl << ", A0.str + A0.str_off[" << sl << "], us" << u << ", ux" << u << ", lane, " << arr
          << (X.eq_dense > 0 ? ", EQA[wave]" : "") << ");\n";
    }
    // two ordering compares of one column (the bounds of a prefix range) share one fetch of the heads
    for (size_t i = 0; i < g.pre_ord.size(); ++i) {
        const auto& [arr, u, sl] = g.pre_ord[i];
        const std::string us = std::to_string(u), tail = ", us" + us + ", ux" + us + ", lane, ";
        if (i + 1 < g.pre_ord.size() && std::get<1>(g.pre_ord[i + 1]) == u) {
            ++i;
            const std::string& arr2 = std::get<0>(g.pre_ord[i]);
            const int sl2 = std::get<2>(g.pre_ord[i]);
            o << "  unsigned " << arr << ", " << arr2 << ";\n  { const int l_[2] = {" << sl << ", " << sl2
              << "}; const char* const q_[2] = {A0.str + A0.str_off[" << sl << "], A0.str + A0.str_off[" << sl2
              << "]}; unsigned r_[2];\n    dfmi::utf8_cmp_lits_tile<BLOCK, K, " << X.ord_h << ", 2>(A, " << u
              << ", l_, q_" << tail << "r_);\n    " << arr << " = r_[0]; " << arr2 << " = r_[1]; }\n";
        } else {
            o << "  unsigned " << arr << ";\n  dfmi::utf8_cmp_lit_tile<BLOCK, K, " << X.ord_h << ">(A, " << u << ", "
              << sl << ", A0.str + A0.str_off[" << sl << "]" << tail << arr << ");\n";
        }
    }
    o << loop.str();
    return offs_loaded;
}

// Numeric slots the aggregates' arguments read (the sub-tile form's
// accumulation passes reload exactly these for the selected rows).
std::vector<int> agg_arg_slots(const Plan& P, const Launch& X) {
    std::vector<int> out;
    for (const AggSpec& a : P.aggs) add_prog_slots(out, X, a.prog);
    std::sort(out.begin(), out.end());
    return out;
}

// The operand of a MIN / MAX as agg_key / agg_isnan take it: a Boolean
// argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY) is an integer extreme over 0 / 1.
std::string extreme_operand(const AggSpec& a, const std::string& v) {
    return a.arg_type == DFMI_TYPE_BOOLEAN ? "(unsigned char)((" + v + ") ? 1 : 0)" : v;
}

// ------------------------------------------------------------- aggregates
// Pieces shared by the ungrouped and the GROUP BY kernel. NA counts the
// kernel's accumulators: the plan's aggregates and, grouped, a hidden last one
// (the group's row count: never a MIN, no float sum).

// (the hidden count is no MIN)
bool agg_is_min(const Plan& P, int j) { return j < (int)P.aggs.size() && P.aggs[j].fn == DFMI_AGG_MIN; }

// The kernel's constants, its LDS state S (`grouped`: one per key slot) and
// the is_min[] / fslot[] tables agg_lds_init and agg_block_flush take.
void emit_agg_head(std::ostream& o, const Plan& P, int NA, bool grouped) {
    int NF = 0;
    for (const AggSpec& a : P.aggs) NF += a.fslot >= 0;
    o << "  constexpr int NA = " << NA << ", NF = " << NF;
    if (grouped) o << ", GS = " << P.gslots;
    o << ";\n  __shared__ dfmi::AggLds<NA, NF> S" << (grouped ? "[GS]" : "") << ";\n";
    o << "  const unsigned char is_min[NA] = {";
    for (int j = 0; j < NA; ++j)
        o << (j ? ", " : "") << (agg_is_min(P, j) ? 1 : 0);
    o << "};\n  const int fslot[NF > 0 ? NF : 1] = {";
    bool any = false;
    for (size_t j = 0; j < P.aggs.size(); ++j)
        if (P.aggs[j].fslot >= 0) {
            o << (any ? ", " : "") << j;
            any = true;
        }
    if (!any) o << "0";
    o << "};\n";
}

// The thread's accumulator registers.
void emit_acc_decls(std::ostream& o, const Plan& P, int NA) {
    for (int j = 0; j < NA; ++j)
        o << "  unsigned acnt" << j << " = 0, afl" << j << " = 0;\n  u64 asum" << j << " = 0, akey" << j << " = "
          << (agg_is_min(P, j) ? "~0ull" : "0ull") << ";\n";
}

// The reduction of row `row` (selected: `sel`) at register index k into the
// accumulator registers; exact float sums go to the LDS state `S` directly.
void emit_accumulate(Gen& g, std::ostream& o, const char* S) {
    for (size_t j = 0; j < g.P.aggs.size(); ++j) {
        const AggSpec& a = g.P.aggs[j];
        const Val v = g.emit(a.prog, a.prog->root, a.ord_base, "sel");
        const std::string ok = "ok" + std::to_string(j) + "_";
        o << "    { const bool " << ok << " = sel && (" << v.n << ");\n";
        o << "      acnt" << j << " += " << ok << " ? 1u : 0u;\n";
        if (a.fn == DFMI_AGG_SUM && a.fslot < 0) {
            o << "      asum" << j << " += " << ok << " ? (u64)(" << (is_signed_int(a.arg_type) ? "i64" : "u64") << ")("
              << v.v << ") : 0ull;\n";
        } else if (a.fn == DFMI_AGG_SUM) {
            o << "      afl" << j << " |= " << ok << " ? dfmi::agg_sum_flags(" << v.v << ") : 0u;\n"
              << "      const bool fin_ = " << ok << " && (dfmi::agg_sum_flags(" << v.v
              << ") == dfmi::AGGF_NONNEGZERO) && (" << v.v << ") != 0;\n"
              << "      dfmi::fsum_add(" << S << ".limbs[" << a.fslot << "], &" << S << ".dlo[" << a.fslot << "], &" << S
              << ".dhi[" << a.fslot << "], (double)(" << v.v << "), fin_, lane);\n";
        } else if (a.fn == DFMI_AGG_MIN || a.fn == DFMI_AGG_MAX) {
            const char* cmp = a.fn == DFMI_AGG_MIN ? "<" : ">";
            const std::string xv = extreme_operand(a, v.v);
            o << "      const bool nan_ = dfmi::agg_isnan(" << xv << ");\n"
              << "      afl" << j << " |= " << ok
              << " ? (nan_ ? (unsigned)dfmi::AGGF_NAN : (unsigned)dfmi::AGGF_VALUE) : 0u;\n"
              << "      if (" << ok << " && !nan_) { const u64 k_ = dfmi::agg_key(" << xv << "); if (k_ " << cmp
              << " akey" << j << ") akey" << j << " = k_; }\n";
        }
        o << "    }\n";
    }
}

// The wave's accumulator registers into the LDS state `S`.
void emit_wave_flush(std::ostream& o, const Plan& P, int NA, const char* S) {
    for (int j = 0; j < NA; ++j)
        o << "  dfmi::agg_wave_flush<NA, NF>(" << S << ", " << j << ", acnt" << j << ", asum" << j << ", akey" << j << ", "
          << (agg_is_min(P, j) ? "true" : "false") << ", afl" << j << ", lane);\n";
}

// One tile per block: its columns' registers, then (after `lead`) the block
// of the rows at `base`, opened here and closed by the caller: selm, and the
// argument-only columns loaded.
void emit_agg_select(Gen& g, std::ostream& o, const char* lead) {
    const Plan& P = g.P;
    const Launch& X = g.X;
    emit_decls(o, X.pred_slots, X, true);
    emit_decls(o, X.proj_slots, X, !P.pred);
    emit_loads(o, X.pred_slots, X, "(i64)t * (BLOCK * K)", nullptr, true);
    o << lead << "  {\n  const i64 base = (i64)t * (BLOCK * K);\n";
    if (P.pred) {
        g.filtered_cols = false;
        // proj_dense: argument-only columns loaded for every row, in the
        // predicate's memory round trip
        if (X.proj_dense) emit_loads(o, X.proj_slots, X, "base", nullptr, false);
        emit_predicate(g, o, {});
        // argument-only columns, loaded only where selected
        if (!X.proj_dense) emit_loads(o, X.proj_slots, X, "base", "(selm >> k) & 1", false);
    } else {
        o << "  unsigned selm = 0;\n#pragma unroll\n  for (int k = 0; k < K; ++k) selm |= (unsigned)(base + k * BLOCK "
             "+ tid < A.n_rows) << k;\n";
        emit_loads(o, X.proj_slots, X, "base", nullptr, true);
    }
    // arguments over the filtered batch (no validity) or the batch itself
    g.filtered_cols = P.pred != nullptr;
}

// The sub-tile passes of generate_agg (Launch::M > 1).
void emit_agg_subtile_passes(Gen& g, std::ostream& o, int NA) {
    const Plan& P = g.P;
    const Launch& X = g.X;
    const std::vector<int> arg_slots = agg_arg_slots(P, X);
    o << "  constexpr int M = " << X.M << ";\n  constexpr unsigned CAP_ = 256;\n"
      << "  __shared__ unsigned short SLA[WAVES][CAP_];\n  __shared__ u64 WSA[M * K * WAVES];\n"
      << "  unsigned tot_ = 0, nsel_ = 0;\n";
    emit_acc_decls(o, P, NA);
    o << "  dfmi::lds_sync();\n";
    // predicate passes: ballots and the list of selected rows
    o << "  for (int m_ = 0; m_ < M; ++m_) {\n  const i64 base = ((i64)t * M + m_) * (BLOCK * K);\n  {\n";
    g.filtered_cols = false;
    emit_decls(o, X.pred_slots, X, true);
    emit_loads(o, X.pred_slots, X, "base", nullptr, true);
    emit_predicate(g, o, {});
    o << "#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    const u64 w_ = __ballot((selm >> k) & 1);\n"
      << "    if (lane == 0) WSA[(m_ * K + k) * WAVES + wave] = w_;\n"
      << "    if (tot_ + (unsigned)__builtin_popcountll(w_) <= CAP_ && ((w_ >> lane) & 1))\n"
      << "      SLA[wave][tot_ + dfmi::lane_rank(w_)] = (unsigned short)((m_ * K + k) * 64 + lane);\n"
      << "    tot_ += (unsigned)__builtin_popcountll(w_);\n  }\n  }\n  }\n"
      << "  nsel_ = tot_;\n  dfmi::wave_lds_fence();\n";
    // sparse: one lane per selected row
    g.filtered_cols = true;
    o << "  if (tot_ <= CAP_) {\n  for (unsigned r_ = 0; r_ < tot_; r_ += 64) {\n"
      << "    const bool sel = r_ + (unsigned)lane < tot_;\n"
      << "    const unsigned e_ = sel ? (unsigned)SLA[wave][r_ + lane] : 0u;\n"
      << "    const int q_ = (int)(e_ >> 6), ls_ = (int)(e_ & 63u);\n"
      << "    const i64 row = ((i64)t * M + q_ / K) * (BLOCK * K) + (i64)(q_ % K) * BLOCK + 64 * wave + ls_;\n"
      << "    const int k = 0;\n";
    for (int sl : arg_slots) {
        const std::string ct = ctype(X.col_type(X.num_cols[sl]));
        o << "    " << ct << " c" << sl << "[1];\n    c" << sl << "[0] = sel ? ((const " << ct << "*)A.col[" << sl
          << "])[row] : (" << ct << ")0;\n";
    }
    emit_accumulate(g, o, "S");
    o << "  }\n  } else {\n";
    // dense: each sub-tile's arguments reloaded where selected
    o << "  for (int m_ = 0; m_ < M; ++m_) {\n  const i64 base = ((i64)t * M + m_) * (BLOCK * K);\n"
      << "  unsigned selm = 0;\n#pragma unroll\n  for (int k = 0; k < K; ++k)\n"
      << "    selm |= (unsigned)((dfmi::lds_uniform_u64(&WSA[(m_ * K + k) * WAVES + wave]) >> lane) & 1) << k;\n"
      << "  if (!__ballot(selm != 0)) continue;\n";
    emit_decls(o, arg_slots, X, false);
    emit_loads(o, arg_slots, X, "base", "(selm >> k) & 1", false);
    o << "#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    const i64 row = base + k * BLOCK + tid;\n    const bool sel = (selm >> k) & 1;\n";
    emit_accumulate(g, o, "S");
    o << "  }\n  }\n  }\n";
}

// Fused Selection + Aggregate kernel (DFMI_FLAG_EXT_AGGREGATE): no compaction
// and no look-back -- the selected rows' argument values are reduced in
// registers, the block's partial goes to a global accumulator copy
// (jit_skeleton.hip "aggregate extension"). One tile per block; or, for a
// predicate that selected few rows last time (aggregate.cpp, Launch::M > 1),
// M sub-tiles per block: the predicate passes keep only each wave's ballots
// (LDS) and a list of its selected rows, then one lane per selected row loads
// the arguments and accumulates -- one dependent round of loads for the M
// sub-tiles instead of one per tile (a wave whose list overflows reloads its
// arguments per sub-tile, lane-masked). The kernel also counts the selected
// rows (totals[0]), which the host keeps as the query shape's selectivity.
void generate_agg(Gen& g, std::ostream& o) {
    const Plan& P = g.P;
    const Launch& X = g.X;
    const int NA = (int)P.aggs.size();
    const bool subtiles = X.M > 1 && P.pred;
    emit_agg_head(o, P, NA, false);
    o << "  if (wave == 0) dfmi::agg_lds_init<NA, NF>(S, is_min, lane);\n";
    if (P.pred) o << "  __shared__ unsigned NSEL_;\n  if (tid == 0) NSEL_ = 0;\n";
    o << "  const unsigned t = tile_;\n";
    if (subtiles) {
        emit_agg_subtile_passes(g, o, NA);
    } else {
        emit_agg_select(g, o, "  unsigned nsel_ = 0;\n");
        if (P.pred)  // selected rows of this wave's K slices, summed for the host's hint
            o << "#pragma unroll\n  for (int k = 0; k < K; ++k) nsel_ += (unsigned)__builtin_popcountll(__ballot((selm >> k) & 1));\n";
        emit_acc_decls(o, P, NA);
        o << "  dfmi::lds_sync();\n";
        o << "#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
          << "    const i64 row = base + k * BLOCK + tid;\n    const bool sel = (selm >> k) & 1;\n";
        emit_accumulate(g, o, "S");
        o << "  }\n";
    }
    emit_wave_flush(o, P, NA, "S");
    // the selected-row count, sampled: every 64th block adds its count (one
    // global atomic per 64 blocks -- a counter every wave hit would serialise)
    if (P.pred) o << "  if (lane == 0 && nsel_) atomicAdd(&NSEL_, nsel_);\n";
    o << "  dfmi::lds_sync();\n  dfmi::agg_block_flush<NA, NF>(A, S, fslot, is_min, tid);\n";
    // (the coalesced form feeds no selectivity hint: nothing is written to the batch's totals)
    if (P.pred && !X.batched) o << "  if (tid == 0 && NSEL_ && (blockIdx.x & 63u) == 0) atomicAdd(A.totals, (u64)NSEL_);\n";
    if (!subtiles) o << "  }\n";
}

// GROUP BY form of the aggregate kernel (one Boolean / integer key): every
// selected row's slot in the batch's key window (Args::gbase / gwidth, null
// key: slot gwidth) is computed once; then, per slot present in the wave
// (uniform loop), the arguments are reduced over that slot's rows exactly as
// in generate_agg and flushed into the slot's LDS state. A hidden last
// aggregate counts the slot's rows (so a group whose arguments are all null
// still exists). Accumulators: [copies][GS][NA + 1][kAggWords].
void generate_agg_grouped(Gen& g, std::ostream& o) {
    const Plan& P = g.P;
    const int NA = (int)P.aggs.size() + 1;  // + the group's row count
    emit_agg_head(o, P, NA, true);
    o << "  const int nslot = A.gwidth + 1;  // <= GS (host-checked)\n";
    o << "  for (int g_ = wave; g_ < nslot; g_ += WAVES) dfmi::agg_lds_init<NA, NF>(S[g_], is_min, lane);\n";
    o << "  const unsigned t = tile_;\n";
    emit_agg_select(g, o, "");
    // the key of every selected row (evaluated before the aggregates: its
    // errors come first in evaluation order) -> its slot
    o << "  unsigned gsl[K];\n#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    const i64 row = base + k * BLOCK + tid;\n    const bool sel = (selm >> k) & 1;\n";
    {
        const Val kv = g.emit(P.gkey, P.gkey->root, P.gkey_ord, "sel");
        if (P.gkey->type == DFMI_TYPE_BOOLEAN) {
            o << "    gsl[k] = !(" << kv.n << ") ? (unsigned)A.gwidth : ((" << kv.v << ") ? 1u : 0u);\n";
        } else {
            o << "    { const u64 d_ = (u64)(" << (is_signed_int(P.gkey->type) ? "i64" : "u64") << ")(" << kv.v
              << ") - A.gbase;\n"
              << "      gsl[k] = !(" << kv.n << ") ? (unsigned)A.gwidth : (d_ < (u64)A.gwidth ? (unsigned)d_ : ~0u);\n"
              << "      if (sel && gsl[k] == ~0u) dfmi::report_err(A.err, 0, 0, dfmi::ERRK_CAPACITY); }\n";
        }
    }
    o << "  }\n  dfmi::lds_sync();\n";
    o << "  for (int g_ = 0; g_ < nslot; ++g_) {\n"
      << "    bool any_ = false;\n#pragma unroll\n    for (int k = 0; k < K; ++k) any_ |= ((selm >> k) & 1) && gsl[k] == (unsigned)g_;\n"
      << "    if (!__ballot(any_)) continue;\n";
    emit_acc_decls(o, P, NA);
    o << "#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    const i64 row = base + k * BLOCK + tid;\n    const bool sel = ((selm >> k) & 1) && gsl[k] == (unsigned)g_;\n"
      << "    acnt" << NA - 1 << " += sel ? 1u : 0u;\n";
    emit_accumulate(g, o, "S[g_]");
    o << "  }\n";
    emit_wave_flush(o, P, NA, "S[g_]");
    o << "  }\n  dfmi::lds_sync();\n"
      << "  for (int g_ = 0; g_ < nslot; ++g_)\n"
      << "    dfmi::agg_block_flush<NA, NF>(A, S[g_], fslot, is_min, tid, A.agg + ((u64)(blockIdx.x % dfmi::kAggCopies) * GS + "
         "g_) * NA * dfmi::kAggWords);\n  }\n";
}

// Coalesced batches: this block's batch, its local tile index `tile_`, and a
// local copy of the Args with the batch's rows, tiles, look-back status
// segment, totals / error words and buffers (the copy is only ever indexed
// with constants, so it lives in registers: no scratch).
void emit_batched_prologue(std::ostream& o, const Plan& P, const Launch& X) {
    const int np = batch_words(X, (int)P.outs.size());
    o << "  const int b_ = A0.tile_batch[bid_];\n"
      << "  void* const* bp_ = A0.batch_ptrs + (i64)b_ * " << np << ";\n"
      << "  dfmi::Args A = A0;\n"
      << "  A.n_rows = (i64)(u64)bp_[0];\n"
      << "  const u64 tt_ = (u64)bp_[1];\n"
      << "  A.n_tiles = (int)(unsigned)tt_;\n"
      << "  const unsigned tile_ = bid_ - (unsigned)(tt_ >> 32);\n"
      << "  A.totals = (u64*)bp_[2];\n  A.err = (u64*)bp_[3];\n"
      // diagnostics (mode bit 4): the forced look-back timeout in the first
      // batch's own error word, which the coalesced launch's host reads
      << "  if ((A.mode & 16) && blockIdx.x == 0 && tid == 0) atomicMax(A.err, ~(u64)3);\n";
    if (P.pred && P.aggs.empty())  // [ch][tile] status words of this batch's tiles
        o << "  A.status = A0.status + (i64)(tt_ >> 32) * " << (1 + X.utf8_outs.size()) * (size_t)X.spread << ";\n";
    for (size_t s = 0; s < X.num_cols.size(); ++s)
        o << "  A.col[" << s << "] = bp_[" << batch_slot_col((int)s) << "];\n  A.valid[" << s << "] = (const u8*)bp_["
          << batch_slot_col((int)s) + 1 << "];\n";
    for (size_t u = 0; u < X.utf8_cols.size(); ++u) {
        const int b = batch_slot_utf8(X, (int)u);
        o << "  A.offs[" << u << "] = (const int*)bp_[" << b << "];\n  A.bytes[" << u << "] = (const u8*)bp_[" << b + 1
          << "];\n  A.svalid[" << u << "] = (const u8*)bp_[" << b + 2 << "];\n";
    }
    for (size_t oi = 0; oi < P.outs.size(); ++oi) {
        const int b = batch_slot_out(X, (int)oi);
        o << "  A.out[" << oi << "] = bp_[" << b << "];\n  A.out_valid[" << oi << "] = (u8*)bp_[" << b + 1
          << "];\n  A.out_offs[" << oi << "] = (int*)bp_[" << b + 2 << "];\n  A.out_data[" << oi << "] = (u8*)bp_["
          << b + 3 << "];\n  A.out_cap[" << oi << "] = (i64)(u64)bp_[" << b + 4 << "];\n";
    }
}

// ------------------------------------------------- Selection + Projection
// What the pieces of a filtered kernel share.
struct FilterCtx {
    Gen& g;
    std::ostream& o;
    const Plan& P;
    const Launch& X;
    std::vector<int> utf8_out_cols;  // the Utf8 outputs' slots
    std::vector<int> out_slots;      // output_slots(P, X)
    std::string tparams;             // the look-back's template arguments

    FilterCtx(Gen& g_, std::ostream& o_) : g(g_), o(o_), P(g_.P), X(g_.X), out_slots(output_slots(g_.P, g_.X)) {
        for (const auto& uo : X.utf8_outs) utf8_out_cols.push_back(uo.second);
        tparams = std::to_string(X.R) + ", " + std::to_string(X.sleep) + ", " + std::to_string(X.spread) + ", " +
                  std::to_string(X.window);
    }
};

// Compaction offsets (rows + Utf8 bytes): the selection ballots wm and the
// per-channel counts cnt (selm and the Utf8 outputs' offsets in scope).
void emit_counts(const FilterCtx& c) {
    std::ostream& o = c.o;
    o << "  unsigned cnt[NCH][K];\n  u64 wm[K];\n#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    wm[k] = __ballot((selm >> k) & 1);\n    cnt[0][k] = (selm >> k) & 1;\n  }\n";
    for (size_t j = 0; j < c.X.utf8_outs.size(); ++j) {
        const int u = c.X.utf8_outs[j].second;
        o << "#pragma unroll\n  for (int k = 0; k < K; ++k) { const int e_ = dfmi::utf8_end(us" << u << "[k], ux" << u
          << "[k], lane); cnt[" << (j + 1) << "][k] = ((selm >> k) & 1) ? "
          << "(unsigned)(e_ - us" << u << "[k]) : 0u; }\n";
    }
}

// The predicate over the rows at `base` (one tile): selm, the projection-only
// loads (unless late), the selection ballots wm and counts cnt.
void emit_select(const FilterCtx& c) {
    const Launch& X = c.X;
    c.g.filtered_cols = false;
    const bool dense = X.proj_dense && !X.late_proj;
    if (dense) emit_loads(c.o, X.proj_slots, X, "base", nullptr, false);
    emit_predicate(c.g, c.o, c.utf8_out_cols);
    // projection-only columns, loaded only where selected
    if (!dense && !X.late_proj) emit_loads(c.o, X.proj_slots, X, "base", "(selm >> k) & 1", false);
    emit_counts(c);
}

// The null counts of the outputs that can be null (OutSpec::nullable): a
// counter per thread, and its sum into the totals.
void emit_null_counters(const FilterCtx& c) {
    for (size_t oi = 0; oi < c.P.outs.size(); ++oi)
        if (c.P.outs[oi].nullable) c.o << "  unsigned nn" << oi << " = 0;\n";
}
void emit_null_flush(const FilterCtx& c) {
    for (size_t oi = 0; oi < c.P.outs.size(); ++oi)
        if (c.P.outs[oi].nullable)
            c.o << "  { const u64 s_ = dfmi::wave_sum((u64)nn" << oi << "); if (lane == 0 && s_) atomicAdd(&A.totals[8 + "
                << oi << "], s_); }\n";
}

// The numeric / Boolean outputs of one selected row (`k`, `row` and its
// output index `d` in scope; the column registers c<slot>[k]).
void emit_out_values(const FilterCtx& c) {
    std::ostream& o = c.o;
    for (size_t oi = 0; oi < c.P.outs.size(); ++oi) {
        const OutSpec& os = c.P.outs[oi];
        if (os.kind == OutSpec::SKIP || os.kind == OutSpec::UTF8) continue;
        Val v;
        if (os.kind == OutSpec::GATHER) {
            IrNode col;
            col.kind = IR_COL;
            col.col = os.col;
            col.type = c.X.col_type(os.col);
            v = c.g.col(col);
        } else {
            v = c.g.emit(os.prog, os.prog->root, os.ord_base, "true");
        }
        const std::string ct = ctype(os.out_type);
        if (os.nullable)  // compacted validity as bytes (packed after the kernel)
            o << "    { const bool v_ = " << v.n << "; ((u8*)A.out_valid[" << oi << "] + obase)[d] = v_ ? 1 : 0;"
              << " nn" << oi << " += v_ ? 0u : 1u; }\n";
        if (os.out_type == DFMI_TYPE_BOOLEAN)
            o << "    ((u8*)A.out[" << oi << "] + obase)[d] = (" << v.v << ") ? 1 : 0;\n";
        else if (c.X.nt & 2)
            o << "    __builtin_nontemporal_store((" << ct << ")(" << v.v << "), (" << ct << "*)A.out[" << oi
              << "] + obase + d);\n";
        else
            o << "    ((" << ct << "*)A.out[" << oi << "] + obase)[d] = " << v.v << ";\n";
    }
}

// One Utf8 output's gather call (channel j + 1), by Launch::gather.
void emit_gather(const FilterCtx& c, size_t j, const std::string& kb, bool prestaged) {
    std::ostream& o = c.o;
    const Launch& X = c.X;
    const int out = X.utf8_outs[j].first, u = X.utf8_outs[j].second;
    const std::string us = std::to_string(u), tail = ", us" + us + ", ux" + us + ", ";
    if (X.gather == 3)
        o << "  dfmi::utf8_offsets_src<BLOCK, K, NCH>(A, T, " << (j + 1) << ", " << out << ", selm, wm, dst" << tail
          << "lane, wave, " << kb << ");\n";
    else if (X.ring && j == 0)
        o << "  dfmi::utf8_gather_ring<BLOCK, K, NCH, " << X.ring << ">(A, T, 1, " << u << ", " << out << ", selm, dst"
          << tail << "RG, lane, wave, tid);\n";
    else if (X.gather == 0)
        o << "  dfmi::utf8_gather_lane<BLOCK, K, NCH>(A, T, " << (j + 1) << ", " << u << ", " << out << ", selm, dst"
          << tail << "lane, wave, " << kb << ");\n";
    else if (X.gather == 6)
        o << "  dfmi::utf8_gather_direct<BLOCK, K, NCH, " << X.direct_grp << ">(A, T, " << (j + 1) << ", " << u << ", "
          << out << ", selm, dst" << tail << "lane, wave, " << kb << ");\n";
    else if (X.gather == 2)
        o << "  dfmi::utf8_gather_serial<BLOCK, K, NCH, ARENA>(A, T, " << (j + 1) << ", " << u << ", " << out
          << ", selm, wm, dst" << tail << "G[wave], lane, wave, " << kb << ");\n";
    else
        o << "  dfmi::utf8_gather<BLOCK, K, NCH, ARENA>(A, T, " << (j + 1) << ", " << u << ", " << out
          << ", selm, wm, dst" << tail << "G[wave], lane, wave, " << kb
          << (X.gather == 4 ? (X.pairs ? ", 3" : X.st16 ? ", 4" : ", 1") : X.gather == 5 ? ", 2" : ", 0")
          << (prestaged && j == 0 ? ", pre_" : ", -1") << (X.gather_phases ? ", true" : ", false")
          << (X.dbuf ? ", true" : ", false") << (X.early ? ", true" : "") << ");\n";
}

// Compacted stores of the selected rows at `base` (selm, wm, the Utf8
// offsets and the column registers in scope; the tile's offsets resolved in
// T); `kb`: the rows' first word of the tile.
void emit_outputs(const FilterCtx& c, const std::string& kb, bool prestaged) {
    std::ostream& o = c.o;
    const Launch& X = c.X;
    // byte-light predicates: projection-only columns after the look-back
    // (fewer registers held across it; few rows are selected)
    if (X.M > 1) emit_loads(o, c.out_slots, X, "base", "(selm >> k) & 1", false);
    else if (X.late_proj) emit_loads(o, X.proj_slots, X, "base", "(selm >> k) & 1", false);
    o << "  const i64 obase = (i64)T.prefix[0];\n  unsigned dst[K];\n#pragma unroll\n"
      << "  for (int k = 0; k < K; ++k) dst[k] = (unsigned)T.excl[0][(" << kb
      << " + k) * WAVES + wave] + dfmi::lane_rank(wm[k]);\n";
    // projections over the selected rows (filtered batch: no validity)
    c.g.filtered_cols = true;
    emit_null_counters(c);
    o << "#pragma unroll\n  for (int k = 0; k < K; ++k) {\n    if (!((selm >> k) & 1)) continue;\n"
      << "    const i64 row = base + k * BLOCK + tid;\n    const unsigned d = dst[k];\n";
    emit_out_values(c);
    o << "  }\n";
    emit_null_flush(c);
    if (X.utf8_outs.empty()) return;
    o << "  if (!(A.mode & 8)) {  // mode bit 3: skip the byte copies (diagnostics)\n";
    for (size_t j = 0; j < X.utf8_outs.size(); ++j) emit_gather(c, j, kb, prestaged);
    o << "  }\n";
}

// The last tile writes every Utf8 output's final offset.
void emit_last_offsets(const FilterCtx& c) {
    if (c.X.utf8_outs.empty()) return;
    c.o << "  if (tid == 0 && t == (unsigned)A.n_tiles - 1) {\n";
    for (size_t j = 0; j < c.X.utf8_outs.size(); ++j)
        c.o << "    A.out_offs[" << c.X.utf8_outs[j].first << "][T.prefix[0] + T.agg[0]] = (int)(T.prefix[" << (j + 1)
            << "] + T.agg[" << (j + 1) << "]);\n";
    c.o << "  }\n";
}

// One tile per block in dispatch order (in order per XCD, so every tile a
// block waits on in the look-back is running or done): predicate,
// projection-only loads, scan + look-back, compacted stores.
void generate_filter_tile(const FilterCtx& c) {
    std::ostream& o = c.o;
    const Launch& X = c.X;
    o << "  __shared__ dfmi::Tile<BLOCK, K, NCH> T;\n";
    emit_decls(o, X.pred_slots, X, true);
    emit_decls(o, X.proj_slots, X, false);
    emit_loads(o, X.pred_slots, X, "(i64)t * (BLOCK * K)", nullptr, true);
    o << "  {\n  const i64 base = (i64)t * (BLOCK * K);\n";
    emit_select(c);
    if (X.ring)  // the loader wave issues the first steps' source bytes now
        o << "  dfmi::ring_prologue<BLOCK, K, " << X.ring << ">(A, RG, " << X.utf8_outs[0].second << ", base, us"
          << X.utf8_outs[0].second << ", lane, wave);\n";
    // the first Utf8 output's first staging round goes out before the
    // look-back, whose wait then hides it
    const bool pre = !X.utf8_outs.empty() && (X.gather == 1 || X.gather >= 4) && X.prestage;
    // (prestage 2: every wave but wave 0, whose look-back polls would
    // otherwise wait behind its staging loads -- vmcnt counts in order)
    if (pre)
        o << "  const int pre_ = " << (X.prestage == 2 ? "wave == 0 ? -1 : " : "") << "dfmi::utf8_gather_prestage<K, "
          << (X.dbuf ? "ARENA / 2" : "ARENA") << ">(A, " << X.utf8_outs[0].second << ", wm, us"
          << X.utf8_outs[0].second << ", ux" << X.utf8_outs[0].second << ", G[wave], lane);\n";
    o << "  dfmi::tile_offsets<BLOCK, K, NCH, " << c.tparams << ">(A, T, t, cnt, lane, wave);\n";
    emit_outputs(c, "0", pre);
    emit_last_offsets(c);
    o << "  }\n";
}

// Sparse output pass of the sub-tile kernel: when the wave's sub-tiles hold
// at most CAP_ selected rows (an equality on a Utf8 column), one lane per
// selected row loads what it needs and stores its outputs -- one round of
// loads for the whole wave instead of one per slice. Leaves the `else` of its
// `if` open for the dense output pass.
void emit_sparse_pass(const FilterCtx& c) {
    std::ostream& o = c.o;
    const Launch& X = c.X;
    // Utf8 outputs: one round of 64 rows (their byte offsets come
    // from one wave scan); numeric outputs: up to 4 rounds
    const int cap = X.utf8_outs.empty() ? 256 : 64;
    o << "  constexpr unsigned CAP_ = " << cap << ";\n"
      << "  __shared__ unsigned short SLR[WAVES][CAP_];\n  unsigned tot_ = 0;\n"
      << "  for (int q_ = 0; q_ < M * K; ++q_) {\n"
      << "    const u64 w_ = dfmi::lds_uniform_u64(&WS[q_ * WAVES + wave]);\n    if (!w_) continue;\n"
      << "    if (tot_ + (unsigned)__builtin_popcountll(w_) <= CAP_ && ((w_ >> lane) & 1))\n"
      << "      SLR[wave][tot_ + dfmi::lane_rank(w_)] = (unsigned short)(q_ * 64 + lane);\n"
      << "    tot_ += (unsigned)__builtin_popcountll(w_);\n  }\n"
      << "  if (tot_ <= CAP_) {\n  dfmi::wave_lds_fence();\n";
    if (cap > 64) o << "  for (unsigned r_ = 0; r_ < tot_; r_ += 64) {\n";
    else o << "  { const unsigned r_ = 0;\n";
    o << "  const bool have_ = r_ + (unsigned)lane < tot_;\n"
      << "  const unsigned e_ = have_ ? (unsigned)SLR[wave][r_ + lane] : 0u;\n"
      << "  const int qs_ = (int)(e_ >> 6), ls_ = (int)(e_ & 63u);\n"
      << "  const i64 row = ((i64)t * M + qs_ / K) * (BLOCK * K) + (i64)(qs_ % K) * BLOCK + 64 * wave + ls_;\n"
      << "  const u64 wq_ = have_ ? WS[qs_ * WAVES + wave] : 0ull;\n"
      << "  const unsigned d = have_ ? (unsigned)T.excl[0][qs_ * WAVES + wave] + "
         "(unsigned)__builtin_popcountll(wq_ & ((1ull << ls_) - 1ull)) : 0u;\n"
      << "  const i64 obase = (i64)T.prefix[0];\n  const int k = 0;\n";
    for (int sl : c.out_slots) {
        const std::string ct = ctype(X.col_type(X.num_cols[sl]));
        o << "  " << ct << " c" << sl << "[1];\n  c" << sl << "[0] = have_ ? ((const " << ct << "*)A.col[" << sl
          << "])[row] : (" << ct << ")0;\n";
    }
    for (size_t j = 0; j < X.utf8_outs.size(); ++j)
        o << "  const int su" << j << "_ = have_ ? A.offs[" << X.utf8_outs[j].second << "][row] : 0, eu" << j
          << "_ = have_ ? A.offs[" << X.utf8_outs[j].second << "][row + 1] : 0;\n";
    c.g.filtered_cols = true;
    emit_null_counters(c);
    o << "  if (have_) {\n";
    emit_out_values(c);
    o << "  }\n";
    emit_null_flush(c);
    if (!X.utf8_outs.empty()) {
        // each selected row's bytes: its slice's byte offset plus the
        // lengths of the selected rows before it in the slice
        o << "  const int qp_ = __builtin_amdgcn_ds_bpermute(((lane + 63) & 63) << 2, qs_);\n"
          << "  const u64 first_ = __ballot(have_ && (lane == 0 || qp_ != qs_));\n"
          << "  const int fl_ = 63 - __builtin_clzll(first_ & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)));\n";
        for (size_t j = 0; j < X.utf8_outs.size(); ++j) {
            const int oo = X.utf8_outs[j].first, u = X.utf8_outs[j].second;
            o << "  { const unsigned L_ = have_ ? (unsigned)(eu" << j << "_ - su" << j << "_) : 0u;\n"
              << "    const unsigned x_ = dfmi::wave_incl_scan32(L_, lane) - L_;\n"
              << "    const unsigned xf_ = (unsigned)__builtin_amdgcn_ds_bpermute(fl_ << 2, (int)x_);\n"
              << "    const u64 ob_ = T.prefix[" << (j + 1) << "] + (have_ ? T.excl[" << (j + 1)
              << "][qs_ * WAVES + wave] : 0ull) + (x_ - xf_);\n"
              << "    if (have_) {\n      A.out_offs[" << oo << "][obase + d] = (int)ob_;\n"
              << "      if ((i64)(ob_ + L_) > A.out_cap[" << oo
              << "]) dfmi::report_err(A.err, 0, 0, dfmi::ERRK_CAPACITY);\n"
              << "      else if (L_ && !(A.mode & 8)) dfmi::utf8_copy(A.bytes[" << u << "] + su" << j << "_, A.out_data["
              << oo << "] + ob_, L_);\n    }\n  }\n";
        }
    }
    o << "  }\n  } else {\n";  // (the rounds; then the dense output pass)
}

// M sub-tiles per block: the predicate pass keeps only each sub-tile's
// ballots and counts (LDS), one scan + look-back covers all of them, and the
// output pass revisits the sub-tiles with selected rows, reloading the Utf8
// offsets and column values they need. (a numeric predicate loads its columns
// per sub-tile; its output pass reloads the columns the outputs read for the
// selected rows only -- chosen for low selectivity, exec_plan.cpp)
void generate_filter_subtiles(const FilterCtx& c) {
    std::ostream& o = c.o;
    const Launch& X = c.X;
    o << "  constexpr int M = " << X.M << ";\n"
      << "  __shared__ dfmi::Tile<BLOCK, K * M, NCH> T;\n  __shared__ u64 WS[K * M * WAVES];\n";
    // software pipeline: sub-tile m+1's Utf8 offsets are loaded while
    // sub-tile m's dependent loads (equality heads) are in flight
    const size_t nu = X.utf8_cols.size();
    for (size_t u = 0; u < nu && X.prefetch; ++u) emit_offs_tile(o, (int)u, "N", "(i64)t * M * (BLOCK * K)", "~0u");

    o << "  for (int m_ = 0; m_ < M; ++m_) {\n  const i64 base = ((i64)t * M + m_) * (BLOCK * K);\n"
      << "  if (base >= A.n_rows) { if (tid < K * WAVES) { WS[m_ * K * WAVES + tid] = 0; }\n"
      << "    for (int c_ = tid; c_ < NCH * K * WAVES; c_ += BLOCK) T.cnt[c_ / (K * WAVES)][m_ * K * WAVES + c_ % (K * WAVES)] = 0;\n"
      << "    continue; }\n";
    for (size_t u = 0; u < nu; ++u)
        if (X.prefetch)
            o << "  int us" << u << "[K], ux" << u << "[K];\n#pragma unroll\n  for (int k = 0; k < K; ++k) { us" << u
              << "[k] = usN" << u << "[k]; ux" << u << "[k] = uxN" << u << "[k]; }\n"
              << "  if (m_ + 1 < M) dfmi::utf8_offs_tile<BLOCK, K>(A, " << u
              << ", base + BLOCK * K, lane, wave, ~0u, usN" << u << ", uxN" << u << ");\n";
        else  // (diagnostics: each sub-tile loads its own offsets when it starts)
            emit_offs_tile(o, (int)u, "", "base", "~0u");
    c.g.filtered_cols = false;
    if (!X.pred_slots.empty()) {
        o << "  {\n";
        emit_decls(o, X.pred_slots, X, true);
        emit_loads(o, X.pred_slots, X, "base", nullptr, true);
    }
    emit_predicate(c.g, o, c.utf8_out_cols, true);
    emit_counts(c);
    o << "  dfmi::subtile_counts<BLOCK, K, NCH>(T, WS, m_ * K, cnt, wm, lane, wave);\n";
    if (!X.pred_slots.empty()) o << "  }\n";
    o << "  }\n";
    o << "  dfmi::tile_scan_lds<BLOCK, K * M, NCH, " << X.spread << ">(A, T, t, lane, wave);\n"
      << "  dfmi::tile_resolve<BLOCK, K * M, NCH, " << c.tparams << ">(A, T, t, lane, wave);\n"
      << "  dfmi::lds_sync();\n";
    // the sparse pass (not with the two-pass gather: its second kernel reads
    // the source starts only the dense pass's utf8_offsets_src writes)
    bool sparse = X.sparse && X.gather != 3;
    for (int sl : c.out_slots) sparse = sparse && X.col_type(X.num_cols[sl]) != DFMI_TYPE_BOOLEAN;
    if (sparse) emit_sparse_pass(c);
    // output pass in steps of KO slices (fewer registers than K)
    o << "  {\n  constexpr int KS = K, K = " << X.KO << ";  // slices per sub-tile / per output step\n"
      << "  for (int q_ = 0; q_ < M * KS; q_ += K) {\n"
      << "  const i64 base = ((i64)t * M + q_ / KS) * (BLOCK * KS) + (i64)(q_ % KS) * BLOCK;\n"
      << "  u64 wm[K];\n  unsigned selm = 0, need_ = 0;\n#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    wm[k] = dfmi::lds_uniform_u64(&WS[(q_ + k) * WAVES + wave]);\n"
      << "    selm |= (unsigned)((wm[k] >> lane) & 1) << k;\n    need_ |= (unsigned)(wm[k] != 0) << k;\n  }\n"
      << "  if (!need_) continue;\n";
    for (int u : c.utf8_out_cols) emit_offs_tile(o, u, "", "base", "need_");
    emit_decls(o, c.out_slots, X, false);
    emit_outputs(c, "q_", false);
    o << "  }\n  }\n";
    if (sparse) o << "  }\n";
    emit_last_offsets(c);
}

// Selection + Projection: the LDS every form shares, then one tile or M sub-tiles.
void generate_filter(Gen& g, std::ostream& o) {
    const FilterCtx c(g, o);
    const Launch& X = c.X;
    o << "  constexpr int NCH = " << 1 + X.utf8_outs.size() << ";\n";
    if (X.ring) o << "  __shared__ dfmi::Utf8Ring<" << X.ring << "> RG;\n";
    if (X.eq_dense > 0) o << "  __shared__ uint4 EQA[WAVES][" << X.eq_dense << "];\n";
    if (!X.utf8_outs.empty() && X.gather && X.gather != 3 && X.gather != 6 && !(X.ring && X.utf8_outs.size() == 1))
        o << "  constexpr int ARENA = " << X.arena << ";\n  __shared__ dfmi::Utf8Stage<ARENA, "
          << (X.gather == 1 ? 32 : X.gather == 5 ? 72 : X.gather == 2 ? 129 : X.image) << "> G[WAVES];\n";
    o << "  const unsigned t = tile_;\n";
    if (X.M == 1) generate_filter_tile(c);
    else generate_filter_subtiles(c);
}

// Projection only: dense rows, ballot-packed validity / Boolean bitmaps.
void generate_project(Gen& g, std::ostream& o) {
    const Plan& P = g.P;
    const Launch& X = g.X;
    o << "  const i64 base = (i64)tile_ * (BLOCK * K);\n";
    std::vector<int> all = X.pred_slots;
    all.insert(all.end(), X.proj_slots.begin(), X.proj_slots.end());
    emit_decls(o, all, X, true);
    emit_loads(o, all, X, "base", nullptr, true);
    o << "  unsigned nulls[" << std::max<size_t>(1, P.outs.size()) << "] = {0};\n";
    o << "#pragma unroll\n  for (int k = 0; k < K; ++k) {\n"
      << "    const i64 row = base + k * BLOCK + tid;\n    const bool in = row < A.n_rows;\n"
      << "    const i64 w = (base >> 6) + k * WAVES + wave;\n";
    for (size_t oi = 0; oi < P.outs.size(); ++oi) {
        const OutSpec& os = P.outs[oi];
        if (os.kind != OutSpec::EXPR) continue;
        const Val v = g.emit(os.prog, os.prog->root, os.ord_base, "in");
        if (os.out_type == DFMI_TYPE_BOOLEAN) {
            o << "    { const u64 vb_ = __ballot(in && (" << v.v << ")); const u64 nb_ = __ballot(in && ("
              << v.n << "));\n"
              << "      nulls[" << oi << "] += __builtin_popcountll(__ballot(in && !(" << v.n << ")));\n"
              << "      if (lane == 0 && w * 64 < A.n_rows) { ((u64*)A.out[" << oi << "])[w] = vb_;"
              << " if (A.out_valid[" << oi << "]) ((u64*)A.out_valid[" << oi << "])[w] = nb_; } }\n";
        } else {
            o << "    if (in) ((" << ctype(os.out_type) << "*)A.out[" << oi << "])[row] = " << v.v << ";\n";
            o << "    { const u64 nb_ = __ballot(in && (" << v.n << "));\n"
              << "      nulls[" << oi << "] += __builtin_popcountll(__ballot(in && !(" << v.n << ")));\n"
              << "      if (lane == 0 && w * 64 < A.n_rows && A.out_valid[" << oi << "]) ((u64*)A.out_valid[" << oi
              << "])[w] = nb_; }\n";
        }
    }
    o << "  }\n";
    for (size_t oi = 0; oi < P.outs.size(); ++oi)
        if (P.outs[oi].kind == OutSpec::EXPR)
            o << "  if (lane == 0 && nulls[" << oi << "]) atomicAdd(&A.totals[8 + " << oi << "], (u64)nulls[" << oi
              << "]);\n";
}

}  // namespace

std::string generate(const Plan& P, Launch& X) {
    X.lits = {};  // (slots are assigned anew by every generation)
    std::ostringstream o;
    Gen g(P, X, o);
    o << "\n// ---- generated query kernel ----\n";
    o << "extern \"C\" __global__ __launch_bounds__(" << X.BLOCK << ")";
    if (X.waves_per_eu > 0) o << " __attribute__((amdgpu_waves_per_eu(" << X.waves_per_eu << ")))";
    o << " void DFMI_KNAME(const dfmi::Args A0) {\n";
    o << "  constexpr int BLOCK = " << X.BLOCK << ", K = " << X.K << ", WAVES = BLOCK / 64;\n";
    o << "  const int tid = threadIdx.x, lane = tid & 63, wave = dfmi::uni(tid >> 6);\n";
    o << "  dfmi::clear_previous<BLOCK>(A0, blockIdx.x, tid);\n";
    if (X.ticket && P.pred && P.aggs.empty())
        o << "  __shared__ unsigned tk_;\n  if (tid == 0) tk_ = atomicAdd(A0.ticket, 1u);\n  __syncthreads();\n"
          << "  const unsigned bid_ = tk_;\n";
    else
        o << "  const unsigned bid_ = blockIdx.x;\n";
    if (X.batched) {
        // (an aggregate: zero outputs in the table; A.agg, gbase and gwidth stay the call's)
        if (!P.aggs.empty() && X.M != 1) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "batched aggregate with sub-tiles"};
        emit_batched_prologue(o, P, X);
    } else {
        o << "  const dfmi::Args& A = A0;\n  const unsigned tile_ = bid_;\n";
    }
    if (!P.aggs.empty() && P.gkey) generate_agg_grouped(g, o);
    else if (!P.aggs.empty()) generate_agg(g, o);
    else if (P.pred) generate_filter(g, o);
    else generate_project(g, o);
    if (X.batched && X.hdr_out)
        // one tile per batch: this block made its batch's whole header (row /
        // byte totals, null counts, error word) -- once every wave's atomics
        // are done, copy it out (the host's pinned result block: no copy
        // back after the kernel) and leave it zero for the next call
        o << "  __threadfence();\n  __syncthreads();\n"
          << "  if (tid < 32) {\n    u64* h_ = (u64*)bp_[2];\n"
          << "    const u64 v_ = __hip_atomic_load(h_ + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
          << "    A0.hdr_out[(i64)b_ * 32 + tid] = v_;\n    h_[tid] = 0;\n  }\n";
    o << "}\n";
    // kernel name: the plan kind and a hash of the whole generated source
    // (prefix, skeleton, body), so that rocprofv3 reports every query shape
    // as its own kernel and a skeleton change renames every kernel (a
    // committed profile never matches code it did not measure)
    std::string body = o.str();
    const std::string prefix = std::string(X.light_copy ? "#define DFMI_LIGHT_COPY 1\n" : "") +
                               (X.long_copy ? "#define DFMI_LONG_COPY " + std::to_string(X.long_copy) + "\n" : "");
    // (the start value is FNV's offset basis less its last digit: kept as it
    // is, since every kernel name, profile and cached code object follows from it)
    static const uint64_t skel_h = fnv1a(skeleton_text().data(), skeleton_text().size(), 1469598103934665603ull);
    const uint64_t h = fnv1a(body.data(), body.size(), fnv1a(prefix.data(), prefix.size(), skel_h));
    char nm[64];
    snprintf(nm, sizeof nm, "dfmi_%s_%08llx", !P.aggs.empty() ? "agg" : (P.pred ? "filter" : "project"),
             (unsigned long long)(h & 0xffffffffull));
    X.kname = nm;
    body.replace(body.find("DFMI_KNAME"), 10, X.kname);
    return prefix + skeleton_text() + body;
}

}  // namespace jit
}  // namespace dfmi
