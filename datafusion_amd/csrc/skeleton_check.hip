// Build-time check of jit_skeleton.hip: instantiates every skeleton template
// with a representative generated body (one Float64 predicate, a gathered
// column, a Utf8 gather, integer division at several widths, the remainder
// helpers at every width, every scalar function helper, every target of the Utf8
// parsers), so a broken skeleton fails `make` rather than the
// first query compile on the GPU. Not linked into libdfmi.so.
#include <hip/hip_runtime.h>

#include "jit_skeleton.hip"

extern "C" __global__ __launch_bounds__(512) void dfmi_skeleton_check(const dfmi::Args A) {
    constexpr int BLOCK = 512, K = 8, WAVES = BLOCK / 64, NCH = 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = dfmi::uni(tid >> 6);
    __shared__ dfmi::Tile<BLOCK, K, NCH> T;
    __shared__ dfmi::Utf8Stage<> G[WAVES];
    const unsigned tile = blockIdx.x;
    const i64 base = (i64)tile * (BLOCK * K);
    const i64 rem = A.n_rows - base;
    u64 c0[K];
    for (int k = 0; k < K; ++k) c0[k] = (k * BLOCK + tid < rem) ? ((const u64*)A.col[0] + base)[k * BLOCK + tid] : 0ull;
    unsigned selm = 0;
    for (int k = 0; k < K; ++k) {
        const i64 row = base + k * BLOCK + tid;
        selm |= (unsigned)(row < A.n_rows && dfmi::f64(c0[k]) > dfmi::f64(A.lits[0])) << k;
    }
    unsigned cnt[NCH][K];
    u64 wm[K];
    int us[K], ue[K];
    bool eq[K];
    dfmi::utf8_offs_tile<BLOCK, K>(A, 0, base, lane, wave, ~0u, us, ue);
    dfmi::utf8_eq_lit_tile<BLOCK, K>(A, 0, 0, A.str + A.str_off[0], us, ue, lane, eq);
    bool eq2[K];
    dfmi::utf8_eq_lit_tile_reg<BLOCK, K, 4>(A, 0, 0, A.str + A.str_off[0], us, ue, lane, eq2);
    for (int k = 0; k < K; ++k) eq[k] = eq[k] || eq2[k];
    // Utf8 ordering: the tile pre-pass at both head widths, the per-row forms
    unsigned o4, o8;
    dfmi::utf8_cmp_lit_tile<BLOCK, K, 4>(A, 0, 0, A.str + A.str_off[0], us, ue, lane, o4);
    dfmi::utf8_cmp_lit_tile<BLOCK, K, 8>(A, 0, 1, A.str + A.str_off[1], us, ue, lane, o8);
    {
        const int l_[2] = {0, 1};
        const char* const q_[2] = {A.str + A.str_off[0], A.str + A.str_off[1]};
        unsigned r_[2];
        dfmi::utf8_cmp_lits_tile<BLOCK, K, 8, 2>(A, 0, l_, q_, us, ue, lane, r_);
        o4 ^= r_[0];
        o8 ^= r_[1];
    }
    for (int k = 0; k < K; ++k) {
        const i64 row = base + k * BLOCK + tid;
        eq[k] = eq[k] || (dfmi::utf8_ord_tile<2>(o4, k) && dfmi::utf8_ord_tile<5>(o8, k)) ||
                dfmi::cmp_opt<3>(dfmi::utf8_valid(A, 0, row), true,
                                 dfmi::utf8_cmp_lit<3, 8>(A, 0, row, 0, A.str + A.str_off[0])) ||
                dfmi::utf8_cmp_lit<4, 4>(A, 0, row, 1, A.str + A.str_off[1]) ||
                dfmi::utf8_cmp_col<2, 8>(A, 0, 1, row) || dfmi::utf8_cmp_col<5, 4>(A, 0, 1, row);
    }
    for (int k = 0; k < K; ++k) {
        selm |= (unsigned)eq[k] << k;
        wm[k] = __ballot((selm >> k) & 1);
        cnt[0][k] = (selm >> k) & 1;
        cnt[1][k] = ((selm >> k) & 1) ? (unsigned)(dfmi::utf8_end(us[k], ue[k], lane) - us[k]) : 0u;
    }
    dfmi::tile_offsets<BLOCK, K, NCH, 4, 2, 16>(A, T, tile, cnt, lane, wave);
    const i64 obase = (i64)T.prefix[0];
    unsigned dst[K];
    for (int k = 0; k < K; ++k) dst[k] = (unsigned)T.excl[0][k * WAVES + wave] + dfmi::lane_rank(wm[k]);
    for (int k = 0; k < K; ++k)
        if ((selm >> k) & 1) ((u64*)A.out[0] + obase)[dst[k]] = c0[k];
    dfmi::utf8_gather<BLOCK, K, NCH, dfmi::kStageChunks>(A, T, 1, 0, 1, selm, wm, dst, us, ue, G[wave], lane, wave);
    dfmi::utf8_gather_serial<BLOCK, K, NCH, dfmi::kStageChunks>(A, T, 1, 0, 1, selm, wm, dst, us, ue, G[wave], lane, wave);
    dfmi::utf8_gather_lane<BLOCK, K, NCH>(A, T, 1, 0, 1, selm, dst, us, ue, lane, wave);
    dfmi::utf8_offsets_src<BLOCK, K, NCH>(A, T, 1, 1, selm, wm, dst, us, ue, lane, wave);
    const bool b = dfmi::cmp_opt<2>(true, false, false) && dfmi::utf8_eq_lit(A, 0, base, 0, A.str) &&
                   dfmi::utf8_eq_col(A, 0, 1, base) && dfmi::utf8_valid(A, 0, base);
    if (b) dfmi::report_err(A.err, 1, base, dfmi::ERRK_DIV_ZERO);
    if (tid == 0 && dfmi::bitmap_word(A.valid[0], 0, A.n_rows) == 7)
        A.totals[0] = (u64)dfmi::idiv<i64>((i64)A.lits[1], (i64)A.lits[2]) +
                      (u64)dfmi::idiv<i8>((i8)A.lits[1], dfmi::int_min<i8>()) + dfmi::idiv<u16>((u16)A.lits[1], 3);
    // Modulus extension: the general and the literal-divisor remainder at every width
    if (tid == 1 && dfmi::bitmap_word(A.valid[0], 0, A.n_rows) == 7) {
        const u64 x = A.lits[1], y = A.lits[2], m = A.lits[4];
        A.totals[1] = (u64)dfmi::irem<i64>((i64)x, (i64)y) + dfmi::irem<u64>(x, y) + (u64)dfmi::irem<i32>((i32)x, (i32)y) +
                      dfmi::irem<u32>((u32)x, (u32)y) + (u64)dfmi::irem<i16>((i16)x, (i16)y) +
                      dfmi::irem<u16>((u16)x, (u16)y) + (u64)dfmi::irem<i8>((i8)x, (i8)y) + dfmi::irem<u8>((u8)x, (u8)y);
        A.totals[2] = (u64)dfmi::irem_lit<i64>((i64)x, (i64)y, m) + dfmi::irem_lit<u64>(x, y, m) +
                      (u64)dfmi::irem_lit<i32>((i32)x, (i32)y, m) + dfmi::irem_lit<u32>((u32)x, (u32)y, m) +
                      (u64)dfmi::irem_lit<i16>((i16)x, (i16)y, m) + dfmi::irem_lit<u16>((u16)x, (u16)y, m) +
                      (u64)dfmi::irem_lit<i8>((i8)x, (i8)y, m) + dfmi::irem_lit<u8>((u8)x, (u8)y, m);
        dfmi::report_err(A.err, 2, base, dfmi::ERRK_REM_OVERFLOW);
    }
    // CAST from Utf8 (DFMI_FLAG_EXT_CAST_ANY): every target's parser through the per-row fetch
    {
        bool lim = false, l2 = false, pb = false;
        i8 a8; i16 a16; i32 a32; i64 a64; u8 b8; u16 b16; u32 b32; u64 b64; float pf; double pd;
        const i64 row = base + tid;
        u64 acc = 0;
        acc += dfmi::utf8_parse<i8>(A, 0, row, a8, l2) ? (u64)a8 : 1;
        acc += dfmi::utf8_parse<i16>(A, 0, row, a16, l2) ? (u64)a16 : 1;
        acc += dfmi::utf8_parse<i32>(A, 0, row, a32, l2) ? (u64)a32 : 1;
        acc += dfmi::utf8_parse<i64>(A, 0, row, a64, l2) ? (u64)a64 : 1;
        acc += dfmi::utf8_parse<u8>(A, 0, row, b8, l2) ? (u64)b8 : 1;
        acc += dfmi::utf8_parse<u16>(A, 0, row, b16, l2) ? (u64)b16 : 1;
        acc += dfmi::utf8_parse<u32>(A, 0, row, b32, l2) ? (u64)b32 : 1;
        acc += dfmi::utf8_parse<u64>(A, 0, row, b64, l2) ? b64 : 1;
        acc += dfmi::utf8_parse<bool>(A, 0, row, pb, l2) ? (u64)pb : 2;
        acc += dfmi::utf8_parse<float>(A, 1, row, pf, l2) ? (u64)__builtin_bit_cast(u32, pf) : 3;
        if (l2) dfmi::report_err(A.err, 3, row, dfmi::ERRK_CAST_DIGITS_F32);
        acc += dfmi::utf8_parse<double>(A, 1, row, pd, lim) ? dfmi::bits(pd) : 4;
        if (lim) dfmi::report_err(A.err, 3, row, dfmi::ERRK_CAST_DIGITS);
        if (row < A.n_rows) ((u64*)A.out[3])[row] = acc;
    }
    // scalar function extension: every helper, Float64 and Float32
    {
        const double x = dfmi::f64(c0[0]), y = dfmi::f64(A.lits[3]);
        const float xf = __builtin_bit_cast(float, (u32)c0[1]), yf = __builtin_bit_cast(float, (u32)A.lits[3]);
        const double d = dfmi::fn_mod<double>(
            dfmi::fn_sqrt<double>(x) + dfmi::fn_abs<double>(x) + dfmi::fn_floor<double>(x) + dfmi::fn_ceil<double>(x) +
                dfmi::fn_round<double>(x) + dfmi::fn_trunc<double>(x), y);
        const float f = dfmi::fn_mod<float>(
            dfmi::fn_sqrt<float>(xf) + dfmi::fn_abs<float>(xf) + dfmi::fn_floor<float>(xf) + dfmi::fn_ceil<float>(xf) +
                dfmi::fn_round<float>(xf) + dfmi::fn_trunc<float>(xf), yf);
        if (base + tid < A.n_rows) {
            ((double*)A.out[1])[base + tid] = d;
            ((float*)A.out[2])[base + tid] = f;
        }
    }
}
