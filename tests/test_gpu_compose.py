"""GPU tests of composed expressions: trees that cross the extension families
(scalar functions, Modulus, CAST from Utf8 and Boolean, Utf8 ordering) through
every kernel form that wraps the query compiler's emitter -- the filtered and
projection-only kernels, the forced sub-tile form with its reloading output
pass, the coalesced-batch forms, the aggregate and grouped kernels, the sort's
fused key pass -- bit for bit.

Expected values come from tests/compose_cases.py: each family's own
restatement composed bottom-up with the oracle (`lower`), pinned on the
families' own expectations and checked seed by seed in
tests/test_compose_cpu.py. The device is never compared with itself. Per
output column: type, length, null count, validity, the values of valid slots,
zero value slots under nulls, the bytes of passed-through Utf8 columns. A
failing assertion names the seed and the query."""
import numpy as np
import pytest

import compose_cases as cc
from compose_cases import A, DI, DX, FL, FLA, FLS, I, S, SCHEMA, U, X, Y
from datafusion_amd import _abi
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.context import Sort, TableScan
from datafusion_amd.execution.engine import engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import (BinaryExpr, Cast, Column, DataType, Float64, Int64, IsNull, Literal, Operator,
                                        SortExpr)
from oracle_ffi import oracle_aggregate, oracle_aggregate_grouped_multi
from test_gpu_cast_any import Str, agg_tuple
from test_gpu_sort import Col, check as check_sorted, expected_order, pull_all
from test_gpu_utf8_order import lit as str_lit

pytestmark = pytest.mark.gpu

U8, BOOL, I64, F64 = DataType.Utf8, DataType.Boolean, DataType.Int64, DataType.Float64
_want = {}   # (query key, rows) -> the expected columns, computed once and never changed


def last_kernel():
    """The name of the query kernel launched last: its kind and a hash of its source."""
    return _abi.lib().dfmi_last_kernel_name(engine().ctx).decode()


def describe(seed, pred, projs):
    return "seed %s: WHERE %r SELECT %s" % (seed, pred, ", ".join(repr(p) for p in projs))


def want_of(key, tab, pred, projs):
    if key not in _want:
        _want[key] = cc.expected(tab, pred, projs)
    return _want[key]


def programs(schema, pred, projs, flags=FL):
    p = compile_scalar_expr(None, pred, schema, flags) if pred is not None else None
    return p, [compile_scalar_expr(None, e, schema, flags) for e in projs]


def ran(what, call):
    """call(), an error it raises reported with the query."""
    try:
        return call()
    except ExecutionError as e:
        raise AssertionError("%s: raised %s: %s" % (what, e.kind, e.message))


def assert_columns(got, want, projs, what):
    assert len(got) == len(want), what
    for j, (g, w, e) in enumerate(zip(got, want, projs)):
        g = g.cpu()
        at = "%s [column %d]" % (what, j)
        if isinstance(w, Str):  # a passed-through Utf8 column
            n, ok = len(w.strings), w.valid
            assert g.data_type == U8 and g.length == n, at
            assert g.null_count == int(n - ok.sum()) and np.array_equal(g.valid_mask(), ok), at
            assert g.numpy_values() == w.strings, at  # (the bytes of null rows too)
            continue
        assert g.data_type == w.data_type and g.length == w.length, (at, g.data_type, g.length, w.length)
        assert g.null_count == w.null_count, (at, g.null_count, w.null_count)
        ok = w.valid_mask()
        assert np.array_equal(g.valid_mask(), ok), (at, np.flatnonzero(g.valid_mask() != ok)[:5])
        gv, wv = np.ascontiguousarray(g.numpy_values()), np.ascontiguousarray(w.numpy_values())
        if w.data_type != BOOL:
            gv, wv = gv.view("u%d" % gv.dtype.itemsize), wv.view("u%d" % wv.dtype.itemsize)
        bad = np.flatnonzero((gv != wv) & ok)
        assert not len(bad), (at, [(int(r), gv[r], wv[r]) for r in bad[:5]])
        if not isinstance(e, Column):  # (a passed-through column keeps its raw slots)
            assert not gv[~ok].any(), (at, "value slots of nulls are not zero", np.flatnonzero((gv != 0) & ~ok)[:5])


def groups_of(seeds, k=6):
    return [seeds[i:i + k] for i in range(0, len(seeds), k)]


def run_plain(seeds, n, query=cc.gen_query):
    """The queries of `seeds` as plain device calls; returns the kernels' names."""
    names = []
    tab = cc.value_table(n)
    batch = tab.device_batch()
    for seed in seeds:
        pred, projs = query(seed)
        want = want_of((seed, n), tab, pred, projs)
        p, cp = programs(SCHEMA, pred, projs)
        what = describe(seed, pred, projs)
        got = ran(what, lambda: engine().filter_project(p, cp, batch, FL))
        names.append(last_kernel())
        assert_columns(got, want, projs, what)
    return names


# ---------------------------------------------------- 1. filter + project, plain
@pytest.mark.parametrize("seeds", groups_of(cc.SEEDS), ids=lambda s: "seeds_%d" % s[0])
def test_filter_project(seeds):
    """4,109 rows: more than one tile with a ragged tail."""
    run_plain(seeds, cc.ROWS)


def test_filter_project_of_a_partial_tile():
    run_plain(cc.SMALL_SEEDS, cc.ROWS_SMALL)


def test_seven_cross_family_trees():
    """floor(CAST(s AS DOUBLE)) % 7.0, sqrt(abs(CAST(a % di AS DOUBLE))),
    CAST(a % 3 = 1 AS INT), CAST(s >= u AS INT), IS NULL(CAST(u AS DOUBLE)),
    CAST(round(x / dx) AS TINYINT) % 5 as one dense query, and again under
    WHERE s < 'm' AND CAST(u AS BIGINT) % 2 = 0."""
    c, lit = Column, lambda v: Literal(Int64(v))
    mod = lambda l, r: BinaryExpr(l, Operator.Modulus, r)
    eq = lambda l, r: BinaryExpr(l, Operator.Eq, r)
    projs = [mod(cc.fn("floor", Cast(c(S), F64)), Literal(Float64(7.0))),
             cc.fn("sqrt", cc.fn("abs", Cast(mod(c(A), c(DI)), F64))),
             Cast(eq(mod(c(A), lit(3)), lit(1)), DataType.Int32),
             Cast(BinaryExpr(c(S), Operator.GtEq, c(U)), DataType.Int32),
             IsNull(Cast(c(U), F64)),
             mod(Cast(cc.fn("round", BinaryExpr(c(X), Operator.Divide, c(DX))), DataType.Int8),
                 Literal(cc.ScalarValue(DataType.Int8, 5)))]
    pred = BinaryExpr(BinaryExpr(c(S), Operator.Lt, str_lit(b"m")), Operator.And,
                      eq(mod(Cast(c(U), I64), lit(2)), lit(0)))
    tab = cc.value_table()
    for name, p in (("dense", None), ("filtered", pred)):
        assert cc.first_error(tab, p, projs) is None
        want = want_of((name, cc.ROWS), tab, p, projs)
        pp, cp = programs(SCHEMA, p, projs)
        what = describe(name, p, projs)
        got = ran(what, lambda: engine().filter_project(pp, cp, tab.device_batch(), FL))
        assert_columns(got, want, projs, what)
    assert 50 < _want[("filtered", cc.ROWS)][0].length < cc.ROWS - 50


# ------------------------------------------------------ 2. the sub-tile form
@pytest.mark.parametrize("case", ["same_seeds", "utf8_free_0", "utf8_free_1"])
def test_forced_subtile_form(case, monkeypatch):
    """DFMI_DIAG=1 DFMI_NUMERIC_SUBTILES=4: the output pass re-evaluates the
    projections from reloaded columns. The form takes queries without a Utf8
    column: those of the seeds above that have none (every other one would run
    the kernel it ran there), and every seed of a Utf8-free list. Every query
    runs another kernel than without the knob."""
    if case == "same_seeds":
        seeds, query = [sd for sd in cc.SEEDS if cc.takes_subtile_form(*cc.gen_query(sd))], cc.gen_query
        assert len(seeds) >= 5
    else:
        seeds, query = cc.SUBTILE_SEEDS[int(case[-1])::2], cc.subtile_query
    plain = run_plain(seeds, cc.ROWS, query)
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_NUMERIC_SUBTILES", "4")
    forced = run_plain(seeds, cc.ROWS, query)
    assert not [sd for sd, a, b in zip(seeds, plain, forced) if a == b], (plain, forced)


# ---------------------------------------------------- 3. coalesced batches
SIZES = [1, 64, 4044, 0]


def batch_expectations(seed, pred, projs):
    parts = cc.split_table(cc.value_table(), SIZES)
    return parts, [want_of((seed, "batch", j), t, pred, projs) for j, t in enumerate(parts)]


@pytest.mark.parametrize("seeds", groups_of(cc.SEEDS, 8), ids=lambda s: "seeds_%d" % s[0])
@pytest.mark.parametrize("form", ["device", "host"])
def test_coalesced_batches(form, seeds):
    """One call over batches of 1, 64, 4,044 rows and an empty one; each batch
    against its own expectation."""
    assert sum(SIZES) == cc.ROWS
    for seed in seeds:
        pred, projs = cc.gen_query(seed)
        parts, want = batch_expectations(seed, pred, projs)
        p, cp = programs(SCHEMA, pred, projs)
        what = describe(seed, pred, projs)
        if form == "device":
            results, err = ran(what, lambda: engine().filter_project_batches(p, cp, [t.device_batch() for t in parts], FL))
        else:
            results, err = ran(what, lambda: engine().filter_project_host_batches(p, cp, [t.host_batch() for t in parts], FL))
            results = [r.materialize() for r in results] if err is None else results
        assert err is None and len(results) == len(SIZES), (what, err)
        for j, (res, w) in enumerate(zip(results, want)):
            assert_columns(res, w, projs, "%s batch %d (%s)" % (what, j, form))


# --------------------------------------------------- 4. aggregate arguments
def run_aggregate(seed, subtile=False):
    """One seed's aggregates against the oracle; returns the kernel's name."""
    tab = cc.value_table()
    pred, tree = cc.gen_numeric_tree(seed, subtile=subtile)
    aggs = cc.aggregates_of(tree)
    key = (seed, "agg")
    if key not in _want:
        _, la, t = cc.lowered_aggregates(tab, pred, aggs)
        _want[key] = agg_tuple(oracle_aggregate(t.schema, t.oracle_batch(), None, la, FLA & ~cc.EXT))
    what = describe(seed, pred, aggs)
    st = engine().agg_state([compile_expr(None, a, SCHEMA, FLA) for a in aggs])
    ran(what, lambda: st.add(compile_scalar_expr(None, pred, SCHEMA, FLA) if pred is not None else None, tab.device_batch(),
                             FLA))
    name = last_kernel()
    got = agg_tuple(ran(what, st.finish))
    assert got == _want[key], (what, got, _want[key])
    return name


@pytest.mark.parametrize("seeds", groups_of(cc.AGG_SEEDS), ids=lambda s: "seeds_%d" % s[0])
def test_aggregates_of_a_generated_tree(seeds):
    """SUM / MIN / MAX / COUNT of a numeric tree under a generated predicate, ungrouped."""
    for seed in seeds:
        run_aggregate(seed)


@pytest.mark.parametrize("seeds", groups_of(cc.AGG_SUBTILE_SEEDS, 4), ids=lambda s: "seeds_%d" % s[0])
def test_aggregates_of_a_generated_tree_subtiles(seeds, monkeypatch):
    """DFMI_DIAG=1 DFMI_AGG_SUBTILES=4 applies to a query with a predicate and
    without a Utf8 or Boolean column: none of the seeds above, every seed of a
    list generated so. Each runs plain, then forced: another kernel, the same bits."""
    plain = [run_aggregate(seed, True) for seed in seeds]
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_AGG_SUBTILES", "4")
    forced = [run_aggregate(seed, True) for seed in seeds]
    assert not [sd for sd, a, b in zip(seeds, plain, forced) if a == b], (plain, forced)


def test_seventeen_literals_in_both_forms_of_the_aggregate_kernel(monkeypatch):
    """SUM / COUNT(x + 1.0 + ... + 17.0) WHERE a > 0, reduced from seed 28106:
    the sub-tile form emits the argument twice and once took a second set of
    literal slots for it, 36 where 32 is the limit."""
    tab = cc.value_table()
    pred, chain = cc.literal_chain()
    aggs = [cc.AggregateFunction("SUM", (chain,), F64), cc.AggregateFunction("COUNT", (Column(A),), DataType.UInt64)]
    _, la, t = cc.lowered_aggregates(tab, pred, aggs)
    want = agg_tuple(oracle_aggregate(t.schema, t.oracle_batch(), None, la, FLA & ~cc.EXT))
    names = []
    for form in ("one tile", "sub-tiles"):
        st = engine().agg_state([compile_expr(None, a, SCHEMA, FLA) for a in aggs])
        ran(form, lambda: st.add(compile_scalar_expr(None, pred, SCHEMA, FLA), tab.device_batch(), FLA))
        names.append(last_kernel())
        assert agg_tuple(ran(form, st.finish)) == want, form
        monkeypatch.setenv("DFMI_DIAG", "1")
        monkeypatch.setenv("DFMI_AGG_SUBTILES", "4")
    assert names[0] != names[1], names


# ----------------------------------------------------- 5. GROUP BY a generated key
@pytest.mark.parametrize("seeds", [cc.GROUP_SEEDS[0::2], cc.GROUP_SEEDS[1::2]], ids=["window", "hash_table"])
def test_group_by_a_generated_key(seeds):
    """(CAST(abs(tree) AS BIGINT) % 1000 + i) % 16: the fused key window, whose
    last kernel is the grouped aggregate kernel; a Float64 tree: the hash
    table, whose last query kernel is its fused Selection + Projection pass."""
    tab = cc.value_table()
    aggs = [cc.AggregateFunction("COUNT", (Column(A),), DataType.UInt64),
            cc.AggregateFunction("SUM", (Cast(Column(cc.F), I64),), I64),
            cc.AggregateFunction("MIN", (Cast(Column(Y), F64),), F64)]
    for seed in seeds:
        pred, key = cc.gen_group_key(seed, seed % 2 == 0)
        what = describe(seed, pred, [key])
        ks, la, t = cc.lowered_aggregates(tab, pred, aggs, [key])
        rk, rv, _ = oracle_aggregate_grouped_multi(t.schema, t.oracle_batch(), None, ks, la, FLA & ~cc.EXT)
        st = engine().grouped_agg_state([compile_scalar_expr(None, key, SCHEMA, FLA)],
                                        [compile_expr(None, a, SCHEMA, FLA) for a in aggs])
        ran(what, lambda: st.add(compile_scalar_expr(None, pred, SCHEMA, FLA) if pred is not None else None,
                                 tab.device_batch(), FLA))
        assert last_kernel().startswith("dfmi_agg_") == (seed % 2 == 0), (what, last_kernel())
        dk, dv = ran(what, st.finish)
        assert len(dk) == len(rk) >= 4, (what, len(dk), len(rk))
        for g in range(len(rk)):
            assert agg_tuple(dk[g]) == agg_tuple(rk[g]), (what, g)
            assert agg_tuple(dv[g]) == agg_tuple(rv[g]), (what, g)


# ----------------------------------------------------- 6. ORDER BY a generated key
@pytest.mark.parametrize("seeds", groups_of(cc.ORDER_SEEDS, 4), ids=lambda s: "seeds_%d" % s[0])
def test_order_by_a_generated_key(seeds):
    """ASC and DESC, the row index and a nullable column as payloads: a null
    key is greater than every value, ties keep the input order."""
    tab = cc.value_table()
    n = tab.rows()
    payload = [Col(I64, np.arange(n)), Col(I64, np.array(tab.cols[A].numpy_values()), tab.cols[A].valid_mask())]
    for seed in seeds:
        key = cc.order_key(seed)
        (k,) = want_of((seed, "order"), tab, None, [key])
        kcol = Col(k.data_type, np.array(k.numpy_values()), k.valid_mask())
        for asc in (True, False):
            ctx = ExecutionContext(flags=FLS)
            ctx.register_datasource("t", MemoryDataSource(SCHEMA, [tab.device_batch()]))
            what = "seed %d: ORDER BY %r %s" % (seed, key, "ASC" if asc else "DESC")
            (rb,) = ran(what, lambda: pull_all(ctx.execute(Sort([SortExpr(key, asc)], TableScan("t", SCHEMA), SCHEMA))))
            try:
                check_sorted([rb.columns[I], rb.columns[A]], payload, expected_order(payload + [kcol], [(2, asc)]))
            except AssertionError as e:
                raise AssertionError("%s: %s" % (what, e))


# ------------------------------------------------------------- 7. error order
ERROR_CASES = cc.error_cases()


@pytest.mark.parametrize("case", ERROR_CASES, ids=[c[0] for c in ERROR_CASES])
def test_the_first_error_across_families(case):
    """Two or three fallible nodes of different families at known ordinals
    with planted failing rows: the reference's first error, from the device
    batch and through the host form."""
    name, tab, pred, projs, planted = case
    want = cc.first_error(tab, pred, projs)
    assert want == planted
    p, cp = programs(tab.schema, pred, projs)
    what = describe(name, pred, projs)
    runs = [("device", lambda: engine().filter_project(p, cp, tab.device_batch(), FL)),
            ("host", lambda: engine().filter_project_host(p, cp, tab.host_batch(), FL))]
    for form, run in runs:
        if want is None:
            assert_columns(ran(what, run), cc.expected(tab, pred, projs), projs, what + " (%s)" % form)
            continue
        with pytest.raises(ExecutionError) as e:
            run()
        assert (e.value.kind, e.value.message) == want, (what, form)
