"""GPU tests of the scalar function extension (DFMI_FLAG_EXT_SCALAR_FUNCTIONS):
sqrt, abs, floor, ceil, round, trunc and mod through engine().filter_project
and ctx.sql, bit for bit, NaN payloads included.

The oracle executes no function, so the expected values come from a
restatement in this file (numpy on bit views for ordinary values, the NaN and
invalid-operation rules of include/dfmi.h written out) composed with the
oracle for everything around the function: `lower` evaluates each function's
arguments with the oracle as a projection, applies the restatement, appends
the result as a nullable column and replaces the node by that Column; the
function-free query then runs through the oracle. A Selection drops validity
(filter.rs:84-93), so a filtered query is expected in two steps: the oracle's
filter of every column, then the projections (or aggregate arguments and
keys) lowered over that all-valid batch. The device is never compared with
itself."""
import numpy as np
import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.engine import engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import (AggregateFunction, BinaryExpr, Cast, Column, DataType, Float64, Literal,
                                        Operator, ScalarFunction)
from datafusion_amd.sqlplanner import SqlToRel
from oracle_ffi import oracle_aggregate, oracle_aggregate_grouped_multi, oracle_filter_project
from test_gpu_parity import assert_same
from test_gpu_sort import Col, check, expected_order, pull_all

pytestmark = pytest.mark.gpu

FN = _abi.DFMI_FLAG_EXT_SCALAR_FUNCTIONS
AGG = _abi.DFMI_FLAG_EXT_AGGREGATE
UNARY = ["sqrt", "abs", "floor", "ceil", "round", "trunc"]
F64, F32 = DataType.Float64, DataType.Float32
NPT = {F64: (np.float64, np.uint64), F32: (np.float32, np.uint32)}


# ------------------------------------------------------------ the restatement
def restate(name, args):
    """The function over numpy vectors of one float type, as bits of that type."""
    x = np.ascontiguousarray(args[0])
    f, u = (np.float64, np.uint64) if x.dtype == np.float64 else (np.float32, np.uint32)
    w = 8 * x.dtype.itemsize
    sign, quiet = u(1 << (w - 1)), u(1 << (51 if w == 64 else 22))
    default_nan = u(0xFFF8000000000000 if w == 64 else 0xFFC00000)
    xb = x.view(u)
    xnan = np.isnan(x)
    with np.errstate(all="ignore"):
        if name == "abs":
            return (xb & ~sign).view(f)
        if name == "mod":
            y = np.ascontiguousarray(args[1])
            r = np.fmod(x, y).view(u).copy()
            r[np.isinf(x) | (y == 0)] = default_nan  # invalid operation, not an error
            r[np.isnan(y)] = (y.view(u) | quiet)[np.isnan(y)]
            r[xnan] = (xb | quiet)[xnan]  # the left operand first
            return r.view(f)
        if name == "sqrt":
            r = np.sqrt(x).view(u).copy()
            r[x < 0] = default_nan  # -inf too; -0.0 is not < 0
        elif name == "round":  # half away from zero
            t = np.trunc(x)
            r = np.where(np.abs(x - t) >= f(0.5), t + np.copysign(f(1), x), t).astype(f).view(u).copy()
        else:
            r = {"floor": np.floor, "ceil": np.ceil, "trunc": np.trunc}[name](x).view(u).copy()
        r[xnan] = (xb | quiet)[xnan]
        return r.view(f)


def test_restatement_known_answers():
    """The restatement itself, on the values the rules name."""
    d = lambda *v: np.array(v, np.float64)
    b = lambda a: [int(x) for x in np.asarray(a).view(np.uint64)]
    nan = lambda bits: np.array([bits], np.uint64).view(np.float64)
    assert b(restate("round", [d(-0.5, 0.49999999999999994, -0.4, 2.5, 4503599627370495.5)])) == \
        b(d(-1.0, 0.0, -0.0, 3.0, 4503599627370496.0))
    assert b(restate("ceil", [d(-0.5)])) == b(d(-0.0))
    assert b(restate("sqrt", [d(-0.0, -1.0, -np.inf, 4.0)])) == [1 << 63, 0xFFF8 << 48, 0xFFF8 << 48, b(d(2.0))[0]]
    assert b(restate("sqrt", [nan(0xFFF0000000000123)])) == [0xFFF8000000000123]
    assert b(restate("abs", [nan(0xFFF0000000000123)])) == [0x7FF0000000000123]
    assert b(restate("mod", [d(1.0, np.inf, -5.0, 5.0), d(0.0, 3.0, 3.0, np.inf)])) == \
        [0xFFF8 << 48, 0xFFF8 << 48] + b(d(-2.0, 5.0))
    assert b(restate("mod", [nan(0x7FF0000000000AAA), nan(0xFFF8000000000BBB)])) == [0x7FF8000000000AAA]
    assert b(restate("mod", [d(1.0), nan(0xFFF0000000000CCC)])) == [0xFFF8000000000CCC]


# ------------------------------------------------ composition with the oracle
def lower(e, schema, batch, flags):
    """e with every ScalarFunction replaced by a Column of its restated values:
    (e', schema', batch'). Raises what the oracle raises for an argument."""
    if isinstance(e, ScalarFunction) and not isinstance(e, AggregateFunction):
        args = []
        for a in e.args:
            a, schema, batch = lower(a, schema, batch, flags)
            args.append(a)
        cols = [oracle_filter_project(schema, batch, None, [a], flags & ~FN)[0][1] for a in args]
        valid = np.ones(batch.num_rows(), bool)
        for c in cols:
            valid &= c.valid_mask()
        vals = restate(e.name, [np.array(c.numpy_values()) for c in cols]).copy()
        vals[~valid] = 0
        arr = Array.from_numpy(e.return_type, vals, None if valid.all() else valid)
        s2 = Schema(list(schema.fields) + [Field("_f%d" % len(schema.fields), e.return_type, True)])
        return Column(len(schema.fields)), s2, RecordBatch(s2, list(batch.columns) + [arr])
    if isinstance(e, BinaryExpr):
        l, schema, batch = lower(e.left, schema, batch, flags)
        r, schema, batch = lower(e.right, schema, batch, flags)
        return BinaryExpr(l, e.op, r), schema, batch
    if isinstance(e, Cast):
        x, schema, batch = lower(e.expr, schema, batch, flags)
        return Cast(x, e.data_type), schema, batch
    return e, schema, batch


def lower_all(exprs, schema, batch, flags):
    out = []
    for e in exprs:
        e, schema, batch = lower(e, schema, batch, flags)
        out.append(e)
    return out, schema, batch


def filtered(schema, batch, pred, flags):
    """The Selection's output batch: every column filtered, validity dropped."""
    if pred is None:
        return schema, batch
    p, s2, b2 = lower(pred, schema, batch, flags)
    cols = oracle_filter_project(s2, b2, p, [Column(i) for i in range(len(schema.fields))], flags & ~FN)
    s3 = Schema([Field(f.name, f.data_type, False) for f in schema.fields])
    return s3, RecordBatch(s3, [a for _, a in cols])


def expected(schema, batch, pred, projs, flags=FN):
    """Projection(Selection?(batch)) as a list of Arrays."""
    s, b = filtered(schema, batch, pred, flags)
    ps, s, b = lower_all(projs, s, b, flags)
    return [a for _, a in oracle_filter_project(s, b, None, ps, flags & ~FN)]


def device(schema, batch, pred, projs, flags=FN):
    p = compile_scalar_expr(None, pred, schema, flags) if pred is not None else None
    cp = [compile_scalar_expr(None, e, schema, flags) for e in projs]
    return [a.cpu() for a in engine().filter_project(p, cp, batch, flags)]


def assert_null_slots_zero(a: Array):
    v = np.array(a.numpy_values())
    assert not v.view("u%d" % v.dtype.itemsize)[~a.valid_mask()].any()


def fn(name, *args, rt=F64):
    return ScalarFunction(name, tuple(args), rt)


def plan_of(sql, schema, flags):
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(schema, []))
    return SqlToRel(ctx).sql_to_rel(sql)


# ----------------------------------------------------------------- edge values
def nan_of(t, negative, quiet, payload):
    f, u = NPT[t]
    info = np.finfo(f)
    top, mb = info.bits - 1, info.nmant
    bits = (((1 << (top - mb)) - 1) << mb) | ((1 << (mb - 1)) if quiet else 0) | payload | ((1 << top) if negative else 0)
    return np.array([bits], u).view(f)[0]


def edge_values(t):
    f, u = NPT[t]
    info = np.finfo(f)
    mb = info.nmant
    one = lambda bits: np.array([bits], u).view(f)[0]
    ulps = lambda v: [np.nextafter(f(v), f(-np.inf)), f(v), np.nextafter(f(v), f(np.inf))]
    rng = np.random.default_rng(5)
    v = [f(0.0), f(-0.0), one(1), -one(1), one((1 << mb) - 1), -one((1 << mb) - 1), info.tiny, -info.tiny,
         info.max, -info.max, f(np.inf), f(-np.inf)]
    for k in (2, 3, 5, 7, 100, 1000, 4095):  # perfect squares +- 1 ulp
        v += ulps(k * k)
    for x in rng.random(30).astype(f) * f(1000):  # x * x +- 1 ulp
        v += ulps(x * x)
    for x in rng.integers(1, 1 << mb, 6):  # subnormal arguments of sqrt, subnormal operands of mod
        v.append(one(int(x)))
    half_below = np.nextafter(f(0.5), f(0))  # 0.49999999999999994 in Float64
    for x in (0.5, 1.5, 2.5, 3.5, half_below, 0.4, 0.6, 2.0 ** mb - 0.5, 2.0 ** mb, 2.0 ** mb + 1, 2.0 ** (mb + 1),
              2.0 ** (mb - 1) + 0.5, 1e15 if t == F64 else 1e6, 1e308 if t == F64 else 1e38, 3.0, 1.0, 0.1, 123456.789):
        v += [f(x), f(-x)]
    for payload in (0, 1, 0x123, (1 << (mb - 1)) - 1):  # quiet and signalling NaNs of both signs
        for quiet in (True, False):
            if quiet or payload:
                v += [nan_of(t, False, quiet, payload), nan_of(t, True, quiet, payload)]
    return np.array(v, dtype=f)


def mod_operands(t):
    """Every edge value against a list of divisors, equal operands, and the
    largest exponent gap (max finite mod the smallest subnormal)."""
    f, u = NPT[t]
    x = edge_values(t)
    info = np.finfo(f)
    one = lambda bits: np.array([bits], u).view(f)[0]
    d = np.array([f(0.0), f(-0.0), f(np.inf), f(-np.inf), f(3.0), f(-3.0), f(1.0), f(0.1), f(7.5), one(1), one(3),
                  info.tiny, info.max, nan_of(t, False, True, 0x55), nan_of(t, True, False, 0x66)],
                 dtype=f)
    xs = np.concatenate([np.repeat(x, len(d)), x, -x])
    ys = np.concatenate([np.tile(d, len(x)), x, x])
    return xs, ys


@pytest.mark.parametrize("t", [F64, F32], ids=["f64", "f32"])
def test_edge_values(t):
    """All seven functions over one batch of hand-picked values, bit for bit."""
    x = edge_values(t)
    assert 150 <= len(x) <= 250
    mx, my = mod_operands(t)
    for name, cols in [(nm, [x]) for nm in UNARY] + [("mod", [mx, my])]:
        s = Schema([Field("c%d" % i, t, False) for i in range(len(cols))])
        b = RecordBatch(s, [Array.from_numpy(t, c) for c in cols])
        (got,) = device(s, b, None, [fn(name, *[Column(i) for i in range(len(cols))], rt=t)])
        want = restate(name, cols)
        u = NPT[t][1]
        assert got.data_type == t and got.length == len(want) and got.null_count == 0, name
        gb, wb = np.array(got.numpy_values()).view(u), want.view(u)
        bad = np.flatnonzero(gb != wb)
        assert not len(bad), (name, [(cols[0][i], hex(gb[i]), hex(wb[i])) for i in bad[:5]])


# --------------------------------------------------------------- random values
def random_table(n, seed, t=F64, null_frac=0.3):
    f = NPT[t][0]
    rng = np.random.default_rng(seed)
    cols = [(rng.random(n) * 4 - 1).astype(f), (rng.random(n) * 100).astype(f), rng.random(n).astype(f)]
    s = Schema([Field(nm, t, True) for nm in "abc"])
    return s, RecordBatch(s, [Array.from_numpy(t, c, rng.random(n) >= null_frac) for c in cols])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096, 4097, 12289])
def test_random_values_with_nulls(n):
    """Nullable arguments (about 30% nulls): validity, null count, zero value
    slots of nulls, the valid slots bit for bit. 4096 rows are one tile at up
    to 4 loaded columns; 4097 cross it."""
    s, b = random_table(n, 100 + n)
    projs = [fn(nm, Column(0)) for nm in UNARY] + [fn("mod", Column(1), Column(0)),
                                                    fn("sqrt", BinaryExpr(Column(1), Operator.Plus, Column(2)))]
    got = device(s, b, None, projs)
    want = expected(s, b, None, projs)
    for e, g, w in zip(projs, got, want):
        assert_same(g, w, repr(e))
        assert g.null_count == w.null_count and np.array_equal(g.valid_mask(), w.valid_mask())
        assert_null_slots_zero(g)
    if n >= 4096:
        s32, b32 = random_table(n, 200 + n, F32)
        p32 = [fn(nm, Column(0), rt=F32) for nm in UNARY] + [fn("mod", Column(1), Column(0), rt=F32)]
        for e, g, w in zip(p32, device(s32, b32, None, p32), expected(s32, b32, None, p32)):
            assert_same(g, w, repr(e))
            assert_null_slots_zero(g)


# ----------------------------------------------------------------- predicates
PRED_SQL = "SELECT a, c FROM t WHERE sqrt(a) < 0.5 AND floor(b * 10) >= 3"
FLAGS_SQL = FN | _abi.DFMI_FLAG_EXT_CAST


@pytest.mark.parametrize("n", [1000, 12289])
def test_function_in_a_predicate(n):
    """Nullable a: sqrt(NULL) is null and arrow's NULL < x = true selects the
    row; a < 0 gives NaN, which no comparison selects."""
    s, b = random_table(n, 7)
    plan = plan_of(PRED_SQL, s, FLAGS_SQL)
    pred, projs = plan.input.expr, plan.expr
    assert repr(pred) == "sqrt(#0) Lt Float64(0.5) And floor(#1 Multiply CAST(Int64(10) AS Float64)) GtEq " \
                         "CAST(Int64(3) AS Float64)"
    want = expected(s, b, pred, projs, FLAGS_SQL)
    got = device(s, b, pred, projs, FLAGS_SQL)
    a_null = ~b.columns[0].valid_mask()
    assert 0 < want[0].length < n and a_null.sum() > 0
    for g, w in zip(got, want):
        assert_same(g, w)
    ctx = ExecutionContext(flags=FLAGS_SQL)
    ctx.register_datasource("t", MemoryDataSource(s, [b.to(engine().device)]))
    (rb,) = pull_all(ctx.sql(PRED_SQL))
    for g, w in zip(rb.columns, want):
        assert_same(g.cpu(), w, "ctx.sql")


# ------------------------------------------------------------ after a Selection
AFTER_SQL = "SELECT sqrt(a * a + b * b), round(c) FROM t WHERE c < 0.5"


def after_selection_table(n, sel):
    rng = np.random.default_rng(31)
    a = rng.random(n) * 6 - 3
    bb = rng.random(n) * 1e3
    c = rng.random(n) * (0.5 / sel)  # c < 0.5 for about `sel` of the rows
    s = Schema([Field(nm, F64, True) for nm in "abc"])
    return s, RecordBatch(s, [Array.from_numpy(F64, a, rng.random(n) >= 0.3), Array.from_numpy(F64, bb),
                              Array.from_numpy(F64, c, rng.random(n) >= 0.005)])  # (a null c is selected)


def run_after_selection(n, sel):
    s, b = after_selection_table(n, sel)
    plan = plan_of(AFTER_SQL, s, FN)
    want = expected(s, b, plan.input.expr, plan.expr)
    assert 0 < want[0].length < n and want[0].null_count == 0
    got = device(s, b, plan.input.expr, plan.expr)
    for g, w in zip(got, want):
        assert_same(g, w)
    return want[0].length


def test_function_after_a_selection():
    """The Selection drops validity: the functions see the raw bits of the
    selected rows' null slots, and their results are all valid."""
    assert run_after_selection(5000, 0.5) > 1000


def test_function_after_a_selection_subtile_output_pass(monkeypatch):
    """The sub-tile kernel's output pass re-evaluates the projections over
    reloaded columns (about 1% of 20,000 rows selected)."""
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_NUMERIC_SUBTILES", "4")
    assert 50 < run_after_selection(20_000, 0.01) < 600


# ----------------------------------------------------------------- error order
def test_error_order():
    n = 3000
    rng = np.random.default_rng(3)
    a, bb = rng.random(n) + 1, rng.random(n) + 1
    bb[2100] = 0.0
    bb[700] = 0.0
    s = Schema([Field("a", F64, False), Field("b", F64, True)])
    valid = np.ones(n, bool)
    valid[700] = False  # a null zero divisor is no error: row 2100 raises
    b = RecordBatch(s, [Array.from_numpy(F64, a), Array.from_numpy(F64, bb, valid)])
    e = fn("sqrt", BinaryExpr(Column(0), Operator.Divide, Column(1)))
    for pred, projs in ((None, [e]), (BinaryExpr(e, Operator.Lt, Literal(Float64(9.0))), [Column(0)]),
                        (BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.0))), [e])):
        with pytest.raises(ExecutionError) as ref:
            expected(s, b, pred, projs)
        with pytest.raises(ExecutionError) as dev:
            device(s, b, pred, projs)
        assert (dev.value.kind, dev.value.message) == (ref.value.kind, ref.value.message)
        assert dev.value.kind == "ArrowError(DivideByZero)"
    # mod by zero is an invalid operation (NaN), not an error
    m = fn("mod", Column(0), Literal(Float64(0.0)))
    (got,) = device(s, b, None, [m])
    (want,) = expected(s, b, None, [m])
    assert_same(got, want)
    assert np.array_equal(np.array(got.numpy_values()).view(np.uint64), np.full(n, 0xFFF8000000000000, np.uint64))


# ------------------------------------------------------- aggregates and keys
def agg_table(n=5000, seed=17):
    rng = np.random.default_rng(seed)
    v = rng.random(n) * 1e4 + 2.5
    k = rng.random(n)
    w = rng.random(n)
    s = Schema([Field("v", F64, True), Field("k", F64, True), Field("w", F64, False)])
    return s, RecordBatch(s, [Array.from_numpy(F64, v, rng.random(n) >= 0.2), Array.from_numpy(F64, k, rng.random(n) >= 0.1),
                              Array.from_numpy(F64, w)])


def agg_exprs(s):
    v = Column(0)
    return [AggregateFunction("SUM", (fn("sqrt", v),), F64), AggregateFunction("MIN", (fn("floor", v),), F64),
            AggregateFunction("COUNT", (fn("sqrt", v),), DataType.UInt64)]


def lower_aggs(aggs, s, b, flags):
    args, s, b = lower_all([a.args[0] for a in aggs], s, b, flags)
    return [AggregateFunction(a.name, (x,), a.return_type) for a, x in zip(aggs, args)], s, b


WHERE = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.6)))
FLA = FN | AGG | _abi.DFMI_FLAG_EXT_GATHER_ALL


def run_plain_aggregate(pred):
    s, b = agg_table()
    aggs = agg_exprs(s)
    fs, fb = filtered(s, b, pred, FLA)
    la, ls, lb = lower_aggs(aggs, fs, fb, FLA)
    ref = oracle_aggregate(ls, lb, None, la, FLA & ~FN)
    st = engine().agg_state([compile_expr(None, a, s, FLA) for a in aggs])
    st.add(compile_scalar_expr(None, pred, s, FLA) if pred is not None else None, b.to(engine().device), FLA)
    dev = st.finish()
    for a, d, r in zip(aggs, dev, ref):
        assert (d.type, d.is_null, d.count) == (r.type, r.is_null, r.count), repr(a)
        assert r.count > 0 and d.bits == r.bits, (repr(a), hex(d.bits), hex(r.bits))


@pytest.mark.parametrize("where", [False, True])
def test_aggregates_of_functions(where):
    run_plain_aggregate(WHERE if where else None)


def test_aggregates_of_functions_subtiles(monkeypatch):
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_AGG_SUBTILES", "4")
    run_plain_aggregate(WHERE)


@pytest.mark.parametrize("where", [False, True])
def test_group_by_a_function_key(where):
    """GROUP BY floor(k * 16): a Float64 key, the hash-table path; 16 groups and the null key."""
    pred = WHERE if where else None
    s, b = agg_table(seed=19)
    aggs = agg_exprs(s)
    key = fn("floor", BinaryExpr(Column(1), Operator.Multiply, Literal(Float64(16.0))))
    fs, fb = filtered(s, b, pred, FLA)
    (lk,), ls, lb = lower_all([key], fs, fb, FLA)
    la, ls, lb = lower_aggs(aggs, ls, lb, FLA)
    rk, rv, _ = oracle_aggregate_grouped_multi(ls, lb, None, [lk], la, FLA & ~FN)
    st = engine().grouped_agg_state([compile_scalar_expr(None, key, s, FLA)], [compile_expr(None, a, s, FLA) for a in aggs])
    st.add(compile_scalar_expr(None, pred, s, FLA) if pred is not None else None, b.to(engine().device), FLA)
    dk, dv = st.finish()
    tup = lambda vs: [(x.type, x.is_null, x.count, 0 if x.is_null else x.bits) for x in vs]
    assert len(dk) == len(rk) and len(rk) == (16 if where else 17)  # (a Selection drops the key's validity)
    for g in range(len(rk)):
        assert tup(dk[g]) == tup(rk[g]), g
        assert tup(dv[g]) == tup(rv[g]), g


# -------------------------------------------------------------------- ORDER BY
def test_order_by_a_function_key():
    n = 3000
    rng = np.random.default_rng(23)
    v = rng.standard_normal(n) * 100
    v[:40] = np.repeat(rng.standard_normal(20), 2) * np.tile([1.0, -1.0], 20)  # ties of |v|: input order
    rng.shuffle(v)
    valid = np.ones(n, bool)
    valid[[5, 77, 1500, 2999]] = False  # the first four of the ten
    s = Schema([Field("v", F64, True), Field("i", DataType.Int64, False)])
    cols = [Col(F64, v, valid), Col(DataType.Int64, np.arange(n))]
    b = RecordBatch(s, [c.array(0, n) for c in cols])
    flags = FN | _abi.DFMI_FLAG_EXT_SORT | _abi.DFMI_FLAG_EXT_GATHER_ALL
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(s, [b.to(engine().device)]))
    (rb,) = pull_all(ctx.sql("SELECT v, i FROM t ORDER BY abs(v) DESC LIMIT 10"))
    key = Col(F64, restate("abs", [v]), valid)  # abs(NULL) is null: greater than every value, first under DESC
    check(rb.columns, cols, expected_order(cols + [key], [(2, False)], 10))


# ----------------------------------------------------------- coalesced batches
def test_coalesced_host_batches():
    """1,024-row host batches (one empty, one ragged) through the relations
    with the default read-ahead: one device call for all of them, the stream
    equal to the single batch's expected result."""
    sql = "SELECT sqrt(a * a + b * b), round(c), a FROM t WHERE sqrt(a) < 0.5 AND floor(b * 10) >= 3"
    sizes = [1024] * 4 + [0] + [1024] * 4 + [777]
    n = sum(sizes)
    s, whole = random_table(n, 41)
    vals = [np.array(c.numpy_values()) for c in whole.columns]
    masks = [c.valid_mask() for c in whole.columns]
    batches, lo = [], 0
    for sz in sizes:
        batches.append(RecordBatch(s, [Array.from_numpy(F64, v[lo:lo + sz], m[lo:lo + sz]) for v, m in zip(vals, masks)]))
        lo += sz
    plan = plan_of(sql, s, FLAGS_SQL)
    want = expected(s, whole, plan.input.expr, plan.expr, FLAGS_SQL)
    ctx = ExecutionContext(flags=FLAGS_SQL)
    assert ctx.coalesce == 256
    ctx.register_datasource("t", MemoryDataSource(s, batches))
    got = pull_all(ctx.sql(sql))
    assert len(got) == len(sizes) and got[4].num_rows() == 0
    assert sum(rb.num_rows() for rb in got) == want[0].length > 100
    for j, w in enumerate(want):
        parts = [np.array(rb.columns[j].cpu().numpy_values()) for rb in got]
        assert all(rb.columns[j].null_count == 0 for rb in got)
        assert np.array_equal(np.concatenate(parts).view(np.uint64), np.array(w.numpy_values()).view(np.uint64)), j
