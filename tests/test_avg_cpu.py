"""AVG (DFMI_FLAG_EXT_AGG_AVG) without a GPU: the front end's errors, the
planner and the serde round trip, the header, and the host finish -- the
exact sum divided by the count and rounded ONCE (csrc/avg_round.h, the text
the device finish runs too) -- driven through dfmi_agg_merge_partials with
partials built by hand, against exact rationals; the aggregate kernels with
an AVG compiled for gfx950; and the host routine under the sanitizers
(tests/native/avg_round_driver.cpp).

Build-defined and parity unpinned: the reference plans avg
(sqlplanner.rs:296) and executes no Aggregate. All comparisons are bit for
bit."""
import os
import random
import re
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Field, Schema
from datafusion_amd.execution.engine import merge_agg_partials
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_expr
from datafusion_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Float64, Literal, Operator
from test_aggregate_cpu import _agg_jit, _grouped_jit, agg, bits_f32, bits_f64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

AGG = _abi.DFMI_FLAG_EXT_AGGREGATE
AVG = AGG | _abi.DFMI_FLAG_EXT_AGG_AVG
UNIT = 1074            # the digits' unit: 2^-1074
LIMBS = 68             # 32-bit digits of an exact sum (aggh::Partial)
F_NAN, F_PINF, F_NINF, F_NNZ = 1, 2, 4, 8   # AGGF_NAN / PINF / NINF / NONNEGZERO
QNAN64, QNAN32 = 0x7FF8000000000000, 0x7FC00000
DBL_MAX_UNITS = int(Fraction(float(np.finfo(np.float64).max)) * 2 ** UNIT)
FLT_MAX_UNITS = int(Fraction(float(np.finfo(np.float32).max)) * 2 ** UNIT)


# ---------------------------------------------------------------- restatement
def f32_round(q: Fraction) -> np.float32:
    """An exact rational rounded to float32, half to even (the restatement of
    test_aggregate_cpu.f32_round; a zero result keeps q's sign)."""
    if q == 0:
        return np.float32(0.0)
    c = np.float32(float(q))
    best = None
    with np.errstate(over="ignore"):  # (the neighbour above the largest finite value is inf: skipped)
        cands = (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)))
    for cand in cands:
        if not np.isfinite(cand):
            continue
        d = abs(Fraction(float(cand)) - q)
        if best is None or d < best[0] or (d == best[0] and (bits_f32(cand) & 1) == 0):
            best = (d, cand)
    r = best[1]
    if r == 0:
        r = np.float32(-0.0) if q < 0 else np.float32(0.0)
    return r


def avg_bits(total_units: int, n: int, f32: bool, flags: int = F_NNZ):
    """The contract restated: the bits of AVG for an exact sum of
    `total_units` * 2^-1074 over n non-null values with the SUM flags `flags`
    (None: null)."""
    if n == 0:
        return None
    if (flags & F_NAN) or ((flags & F_PINF) and (flags & F_NINF)):
        return QNAN32 if f32 else QNAN64
    if flags & (F_PINF | F_NINF):
        v = float("inf") if flags & F_PINF else float("-inf")
        return bits_f32(v) if f32 else bits_f64(v)
    if total_units == 0:
        v = 0.0 if flags & F_NNZ else -0.0
        return bits_f32(v) if f32 else bits_f64(v)
    q = Fraction(total_units, n << UNIT)
    if f32:
        return bits_f32(f32_round(q))
    v = float(q)  # int / int true division: correctly rounded, subnormals included
    if v == 0.0 and total_units < 0:
        v = -0.0
    return bits_f64(v)


def test_the_restatement_rounds_subnormals_half_to_even():
    # 0.5, 1.5, 2.5 and 1.75 quanta -> 0, 2, 2, 2 quanta
    for num, den, want in ((1, 2, 0), (3, 2, 2), (5, 2, 2), (7, 4, 2)):
        assert bits_f64(float(Fraction(num, den << UNIT))) == want
        assert avg_bits(num, den, False) == want


# ------------------------------------------------------------- hand partials
def digits_of(total: int, rng: random.Random, loose: bool):
    """`total` (units of 2^-1074, signed) as 68 int64 digits: every digit but
    the top in [0, 2^32), the top signed; `loose`: then carries moved between
    neighbouring digits at random, so the digits are not normalised."""
    d = []
    t = total
    for _ in range(LIMBS - 1):
        d.append(t & 0xffffffff)
        t >>= 32  # floor
    d.append(t)
    assert -2 ** 62 < t < 2 ** 62
    if loose:
        for _ in range(rng.randrange(1, 12)):
            i = rng.randrange(0, LIMBS - 1)
            k = rng.randrange(-2 ** 20, 2 ** 20)
            d[i] += k << 32
            d[i + 1] -= k
    assert sum(x << (32 * i) for i, x in enumerate(d)) == total
    return d


def partial(count: int, flags: int, digits) -> bytes:
    """aggh::Partial: count, flags, key, isum, then the 68 digits."""
    return struct.pack("<4Q", count, flags, 0, 0) + struct.pack("<%dq" % LIMBS, *digits)


def split_partials(total: int, n: int, flags: int, rng: random.Random):
    """The state (total, n, flags) split over 1 to 3 partials with loose digits."""
    parts = rng.randrange(1, 4)
    totals, counts = [], []
    for _ in range(parts - 1):
        totals.append(rng.randrange(-abs(total) - 1, abs(total) + 2) if rng.random() < 0.8 else 0)
        counts.append(rng.randrange(0, n + 1 - sum(counts)))
    totals.append(total - sum(totals))
    counts.append(n - sum(counts))
    fl = [flags if i == 0 else (flags if rng.random() < 0.5 else 0) for i in range(parts)]
    return [partial(c, f, digits_of(t, rng, True)) for t, c, f in zip(totals, counts, fl)]


def avg_agg(t: DataType):
    s = Schema([Field("x", t, True)])
    return compile_expr(None, AggregateFunction("AVG", (Column(0),), t), s, AVG)


def finish(a, parts):
    (v,) = merge_agg_partials([a], parts)
    return v


def random_total(rng: random.Random, n: int, limit_units: int, f32: bool) -> int:
    """A signed total whose mean is within the format's finite range: a
    mantissa of 1 to 120 random bits at a random position over the whole
    exponent range (subnormal means, means of a fraction of a quantum, means
    next to the largest finite value)."""
    while True:
        kind = rng.random()
        bits = rng.randrange(1, 121)
        m = rng.getrandbits(bits) | 1
        if kind < 0.15:    # the mean in or below the subnormal range
            lo = (UNIT - 149) if f32 else 0
            t = m * n >> rng.randrange(0, bits + 8) << lo if rng.random() < 0.5 else m << rng.randrange(0, lo + 60)
        elif kind < 0.25:  # exact multiples and exact halves of n (ties)
            t = (2 * m + rng.randrange(0, 2)) * n >> 1 << rng.randrange(0, 1900 if not f32 else 1000)
        else:
            t = m << rng.randrange(0, limit_units.bit_length() + n.bit_length())
        if t and Fraction(t, n) <= limit_units:
            return -t if rng.random() < 0.4 else t


def random_n(rng: random.Random) -> int:
    k = rng.random()
    if k < 0.4:
        return rng.randrange(1, 10)
    if k < 0.6:
        return rng.randrange(1, 2 ** 32)
    if k < 0.8:
        return rng.randrange(2 ** 32, 2 ** 62 + 1)
    return 1 << rng.randrange(0, 63)  # powers of two up to 2^62


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_host_finish_random_totals(f32):
    rng = random.Random(20 + f32)
    a = avg_agg(DataType.Float32 if f32 else DataType.Float64)
    limit = FLT_MAX_UNITS if f32 else DBL_MAX_UNITS
    seen_big_n = seen_sub = 0
    for case in range(3000):
        n = random_n(rng)
        total = random_total(rng, n, limit, f32)
        v = finish(a, split_partials(total, n, F_NNZ, rng))
        want = avg_bits(total, n, f32)
        assert (v.is_null, v.count, v.bits) == (0, n, want), (case, total, n, hex(v.bits), hex(want))
        assert v.type == (DataType.Float32 if f32 else DataType.Float64)
        seen_big_n += n >= 2 ** 32
        seen_sub += (want & 0x7fffffff) < 0x00800000 if f32 else (want & (2 ** 63 - 1)) < 2 ** 52
    assert seen_big_n > 300 and seen_sub > 100


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_host_finish_sums_of_values(f32):
    """Totals that are sums of a few values over the whole exponent range,
    with exact cancellations: n is the number of values."""
    rng = random.Random(30 + f32)
    nrng = np.random.default_rng(30 + f32)
    a = avg_agg(DataType.Float32 if f32 else DataType.Float64)
    for case in range(1500):
        k = rng.randrange(1, 10)
        if f32:
            xs = (nrng.standard_normal(k) * np.exp2(nrng.integers(-149, 127, k))).astype(np.float32).astype(np.float64)
        else:
            xs = np.ldexp(nrng.random(k) + 1.0, nrng.integers(-1074, 1023, k)) * np.where(nrng.random(k) < 0.5, -1, 1)
        xs = list(xs)
        if rng.random() < 0.3:
            xs += [-x for x in xs[: rng.randrange(1, k + 1)]]  # cancels exactly
        total = sum(int(Fraction(float(x)) * 2 ** UNIT) for x in xs)
        n = len(xs)
        flags = F_NNZ
        v = finish(a, split_partials(total, n, flags, rng))
        want = avg_bits(total, n, f32, flags)
        assert (v.is_null, v.count, v.bits) == (0, n, want), (case, xs, hex(v.bits), hex(want))


def test_host_finish_named_cases():
    rng = random.Random(5)
    a64, a32 = avg_agg(DataType.Float64), avg_agg(DataType.Float32)

    def one(a, total, n, flags=F_NNZ):
        return finish(a, [partial(n, flags, digits_of(total, rng, False))])

    # two and three copies of the largest finite value come back as that value
    for k in (2, 3):
        assert one(a64, k * DBL_MAX_UNITS, k).bits == bits_f64(np.finfo(np.float64).max)
        assert one(a32, k * FLT_MAX_UNITS, k).bits == bits_f32(np.finfo(np.float32).max)
    # 1, 3 and 5 quanta over n = 2: 0 (a tie to even), 2, 2 quanta
    for total, want in ((1, 0), (3, 2), (5, 2), (-1, 1 << 63), (-3, (1 << 63) | 2)):
        assert one(a64, total, 2).bits == want
    q32 = 1 << (UNIT - 149)
    for total, want in ((q32, 0), (3 * q32, 2), (5 * q32, 2), (-q32, 1 << 31)):
        assert one(a32, total, 2).bits == want
    # a negative sum whose mean rounds to zero keeps the sum's sign
    assert one(a64, -1, 3).bits == bits_f64(-0.0)
    assert one(a32, -7, 1000).bits == bits_f32(-0.0)
    # an exact-zero sum: -0.0 only if every value is -0.0 (no NONNEGZERO flag)
    assert one(a64, 0, 4, F_NNZ).bits == bits_f64(0.0) and one(a64, 0, 4, 0).bits == bits_f64(-0.0)
    assert one(a32, 0, 4, F_NNZ).bits == bits_f32(0.0) and one(a32, 0, 4, 0).bits == bits_f32(-0.0)
    # no non-null value: null
    v = one(a64, 0, 0, 0)
    assert (v.is_null, v.count) == (1, 0)
    # NaN, +inf, -inf, +inf with -inf (whatever the digits hold)
    for a, f32 in ((a64, False), (a32, True)):
        for flags in (F_NAN | F_NNZ, F_PINF | F_NNZ, F_NINF | F_NNZ, F_PINF | F_NINF | F_NNZ, F_NAN | F_PINF):
            v = one(a, 12345 << 1000, 7, flags)
            assert (v.is_null, v.count, v.bits) == (0, 7, avg_bits(12345 << 1000, 7, f32, flags)), flags
    assert one(a64, 1, 1, F_PINF).bits == bits_f64(float("inf"))
    assert one(a32, 1, 1, F_PINF | F_NINF).bits == QNAN32
    # the largest n: 2^63 - 1 values of 1.0
    n = 2 ** 63 - 1
    assert one(a64, n << UNIT, n).bits == bits_f64(1.0)
    assert one(a64, (n << UNIT) + 1, n).bits == bits_f64(1.0)
    assert one(a64, 1 << UNIT, n).bits == avg_bits(1 << UNIT, n, False)


# ------------------------------------------------------------------ front end
def test_front_end_flag_name_types():
    s = Schema([Field("x", DataType.Float64, False), Field("u", DataType.Utf8, False), Field("i", DataType.Int32, True),
                Field("f", DataType.Float32, True), Field("b", DataType.Boolean, True), Field("w", DataType.UInt64, True)])
    # without the new flag: the reference's panic, as before
    for flags in (AGG, AGG | _abi.DFMI_FLAG_EXT_SCALAR_FUNCTIONS):
        with pytest.raises(ExecutionError) as ei:
            compile_expr(None, agg("avg", Column(0), s), s, flags)
        assert ei.value.kind == "panic"
        assert ei.value.message == "not yet implemented: Unsupported aggregate function 'avg'"
    with pytest.raises(ExecutionError) as ei:  # the new flag alone is not the aggregate extension
        compile_expr(None, agg("avg", Column(0), s), s, _abi.DFMI_FLAG_EXT_AGG_AVG)
    assert (ei.value.kind, ei.value.message) == ("panic", "not yet implemented")
    for name in ("avg", "AVG", "Avg", "aVG"):
        a = compile_expr(None, agg(name, Column(0), s), s, AVG)
        assert a.get_name() == name and a.get_type() == DataType.Float64
    assert compile_expr(None, agg("avg", Column(3), s), s, AVG).get_type() == DataType.Float32
    e = BinaryExpr(Column(0), Operator.Multiply, Literal(Float64(0.5)))
    assert compile_expr(None, agg("AVG", e, s), s, AVG).get_type() == DataType.Float64
    # integers: no exact sum to divide
    for col, tname in ((2, "Int32"), (5, "UInt64")):
        with pytest.raises(ExecutionError) as ei:
            compile_expr(None, agg("AVG", Column(col), s), s, AVG)
        assert ei.value.kind == "NotImplemented"
        assert ei.value.message == "AVG over %s: cast the argument to Float64" % tname
    # Boolean and Utf8 fail as they do for SUM
    for col in (1, 4):
        errs = []
        for name in ("SUM", "AVG"):
            with pytest.raises(ExecutionError) as ei:
                compile_expr(None, agg(name, Column(col), s), s, AVG)
            errs.append((ei.value.kind, ei.value.message))
        assert errs[0] == errs[1] and errs[0][0] == "NotImplemented"
    # the planner's return type is the argument's
    for t in (DataType.Float32, DataType.UInt64, DataType.Int64):
        with pytest.raises(ExecutionError) as ei:
            compile_expr(None, AggregateFunction("AVG", (Column(0),), t), s, AVG)
        assert ei.value.message == "aggregate return type does not match the planner's"
    # the other names are untouched by the flag
    with pytest.raises(ExecutionError) as ei:
        compile_expr(None, agg("median", Column(0), s), s, AVG)
    assert ei.value.message == "not yet implemented: Unsupported aggregate function 'median'"
    assert compile_expr(None, agg("SUM", Column(2), s), s, AVG).get_type() == DataType.Int32


def test_planner_builds_avg_and_serde_round_trip():
    from datafusion_amd.execution import ExecutionContext, MemoryDataSource
    from datafusion_amd.execution.context import Aggregate
    from datafusion_amd.sqlplanner import SqlToRel
    s = Schema([Field("city", DataType.Utf8, False), Field("lat", DataType.Float64, False),
                Field("lng", DataType.Float64, False)])
    ctx = ExecutionContext(flags=AVG)
    ctx.register_datasource("t", MemoryDataSource(s, []))
    p = SqlToRel(ctx).sql_to_rel("SELECT AVG(lat), avg(lng * 2.0) FROM t WHERE lat < 53")
    assert isinstance(p, Aggregate)
    assert [repr(e) for e in p.aggr_expr] == ["AVG(#1)", "avg(#2 Multiply Float64(2.0))"]
    assert [e.return_type for e in p.aggr_expr] == [DataType.Float64, DataType.Float64]
    # (the wire form carries the plan's schema, which the planner leaves to the executor)
    p = Aggregate(p.input, p.group_expr, p.aggr_expr,
                  Schema([Field("AVG", DataType.Float64, True), Field("avg", DataType.Float64, True)]))
    back = serde.from_json(serde.to_json(p))
    assert isinstance(back, Aggregate) and [repr(e) for e in back.aggr_expr] == [repr(e) for e in p.aggr_expr]
    assert [e.return_type for e in back.aggr_expr] == [DataType.Float64, DataType.Float64]
    assert serde.to_json(back) == serde.to_json(p)
    for e in back.aggr_expr:
        assert compile_expr(ctx, e, s).get_type() == DataType.Float64


def test_header_declares_the_flag_and_the_enum_value():
    h = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    assert re.search(r"#define\s+DFMI_FLAG_EXT_AGG_AVG\s+0x80u", h)
    assert re.search(r"DFMI_AGG_AVG\s*=\s*4\b", h)
    assert re.search(r"#define DFMI_ABI_VERSION 4\b", h)
    assert _abi.DFMI_FLAG_EXT_AGG_AVG == 0x80 and _abi.DFMI_AGG_AVG == 4
    assert _abi.DFMI_ABI_VERSION == 4 and _abi.lib().dfmi_abi_version() == 4


# -------------------------------------------------------------------- kernels
def test_aggregate_kernels_with_avg_compile():
    """The ungrouped and the window kernels with an AVG compile for gfx950,
    and their source is the source of the same query with SUM in AVG's place
    (an AVG accumulates as a SUM: one code object)."""
    s = Schema([Field("q", DataType.Float64, False), Field("p", DataType.Float64, True),
                Field("f", DataType.Float32, True), Field("k", DataType.Int16, True)])
    pred = BinaryExpr(Column(0), Operator.Lt, Literal(Float64(24.0)))
    fl = AVG | _abi.DFMI_FLAG_EXT_GATHER_ALL

    def aggs(name):
        return [agg(name, BinaryExpr(Column(0), Operator.Multiply, Column(1)), s), agg(name, Column(2), s),
                agg("COUNT", Column(1), s), agg("MIN", Column(2), s)]
    for p in (None, pred):
        rc, code, msg, src = _agg_jit(s, p, aggs("AVG"), fl)
        assert rc > 0, msg
        assert "fsum_add" in src
        assert src == _agg_jit(s, p, aggs("SUM"), fl, compile_=False)[3]
        rc, code, msg, gsrc = _grouped_jit(s, p, Column(3), aggs("avg"), fl)
        assert rc > 0, msg
        assert gsrc == _grouped_jit(s, p, Column(3), aggs("sum"), fl, compile_=False)[3]
    # four AVGs fill the four float-SUM slots; a fifth is the existing program limit
    four = [agg("AVG", Column(c), s) for c in (0, 1, 2, 0)]
    rc, code, msg, src = _agg_jit(s, None, four, fl, compile_=False)
    assert rc > 0, msg
    rc, code, msg, src = _agg_jit(s, None, four + [agg("AVG", Column(1), s)], fl, compile_=False)
    assert rc < 0 and msg == "device program limit: more than 4 floating-point SUMs"


# ----------------------------------------------------------------- sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_avg_host_finish_under_asan_ubsan(tmp_path):
    out = str(tmp_path / "avg_round_driver")
    csrc = os.path.join(ROOT, "datafusion_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", out,
           os.path.join(HERE, "native", "avg_round_driver.cpp"), os.path.join(csrc, "agg_host.cpp"),
           os.path.join(csrc, "compile.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "avg round driver: clean" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
