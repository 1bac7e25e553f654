"""GPU tests of CAST from Utf8 and Boolean (DFMI_FLAG_EXT_CAST_ANY), bit for bit.

The oracle executes no CAST of a column, so the expected values of a cast come
from the Python restatement of the contract (tests/test_cast_any_cpu.py:
`restate`, pinned there on the corpus, CPython's float() and the native CSV
reader) and never from the device. Everything around the cast comes from the
oracle: `lower` replaces each new-form CAST by a Column holding the restated
values as an ordinary nullable column and runs the cast-free query through the
oracle. A Selection drops validity (filter.rs:84-93), so a filtered query is
expected in two steps: the oracle's filter (the selected rows' indices), then
the projections / aggregate arguments / keys lowered over the selected rows,
whose strings -- null slots too -- are parsed by their raw bytes."""
import numpy as np
import pyarrow as pa
import pytest
import torch

from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema, np_dtype, pack_bits
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.engine import engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import (AggregateFunction, BinaryExpr, Cast, Column, DataType, Float64, Int64, Literal,
                                        Operator)
from datafusion_amd.sqlplanner import SqlToRel
from oracle_ffi import oracle_aggregate, oracle_aggregate_grouped_multi, oracle_filter_project
from test_cast_any_cpu import (BOTH, CORPUS, FLOATS, INTS, LIMIT, LIMIT_STRING, NUMERIC, TARGETS, limit_message,
                               random_strings, restate)
from test_gpu_parity import assert_same
from test_gpu_sort import Col, check, expected_order, pull_all

pytestmark = pytest.mark.gpu

ANY = _abi.DFMI_FLAG_EXT_CAST_ANY
FL = BOTH | _abi.DFMI_FLAG_EXT_GATHER_ALL
AGG = _abi.DFMI_FLAG_EXT_AGGREGATE
FLA = FL | AGG
U8, BOOL, I64, F64 = DataType.Utf8, DataType.Boolean, DataType.Int64, DataType.Float64
NOT_IMPL = "NotImplemented"

_memo = {}


def parse(s, t):
    k = (s, t)
    if k not in _memo:
        _memo[k] = restate(s, t)
    return _memo[k]


class Str:
    """A Utf8 column on the host: its strings -- those of null rows too, which
    keep their bytes -- and its validity."""

    def __init__(self, strings, valid=None):
        self.strings = list(strings)
        self.valid = np.ones(len(self.strings), bool) if valid is None else np.asarray(valid, bool)

    def array(self, device="cpu", pad=0):
        """The data buffer ends at the last string's last byte and begins `pad`
        bytes past a 4-byte boundary."""
        n = len(self.strings)
        flat = np.frombuffer(b"".join(self.strings), np.uint8)
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(s) for s in self.strings])
        big = torch.zeros(pad + max(1, len(flat)), dtype=torch.uint8)
        if len(flat):
            big[pad:pad + len(flat)] = torch.from_numpy(flat.copy())
        big = big.to(device)
        assert big.data_ptr() % 4 == 0
        nulls = int(n - self.valid.sum())
        vb = torch.from_numpy(pack_bits(self.valid)).to(device) if nulls else None
        return Array(U8, n, big[pad:pad + max(1, len(flat))], vb, torch.from_numpy(offs).to(device), nulls)

    def oracle_array(self):
        return Array.from_strings([s if ok else None for s, ok in zip(self.strings, self.valid)])

    def take(self, idx):  # the Selection's output: all valid, the bytes as they are
        return Str([self.strings[i] for i in idx])

    def parsed(self, t):
        """CAST(column AS t) restated: (values, validity, rows at the program limit)."""
        n = len(self.strings)
        vals = np.zeros(n, bool if t == BOOL else ("u%d" % t.width if t in FLOATS else np_dtype(t)))
        ok = np.zeros(n, bool)
        lim = []
        for i, (s, v) in enumerate(zip(self.strings, self.valid)):
            if not v:
                continue
            r = parse(s, t)
            if r is LIMIT:
                lim.append(i)
            elif r is not None:
                vals[i], ok[i] = r, True
        return (vals.view(np_dtype(t)) if t in FLOATS else vals), ok, lim


class Table:
    """Columns by position: Str for Utf8, a host Array for everything else."""

    def __init__(self, fields, cols):
        self.fields, self.cols = list(fields), list(cols)

    @property
    def schema(self):
        return Schema(self.fields)

    def rows(self):
        c = self.cols[0]
        return len(c.strings) if isinstance(c, Str) else c.length

    def oracle_batch(self):
        return RecordBatch(self.schema, [c.oracle_array() if isinstance(c, Str) else c for c in self.cols])

    def device_batch(self, pad=0, device=None):
        device = device or engine().device
        return RecordBatch(self.schema, [c.array(device, pad) if isinstance(c, Str) else c.to(device) for c in self.cols])

    def host_batch(self):
        return self.device_batch(0, "cpu")

    def with_column(self, t, vals, valid):
        a = Array.from_numpy(t, vals, None if valid.all() else valid)
        return Table(self.fields + [Field("_c%d" % len(self.fields), t, True)], self.cols + [a])


def oracle_eval(tab, e):
    return oracle_filter_project(tab.schema, tab.oracle_batch(), None, [e], FL & ~ANY)[0][1]


def lower(e, tab):
    """e with every new-form CAST replaced by a Column of restated values."""
    if isinstance(e, Cast):
        if isinstance(e.expr, Column) and tab.fields[e.expr.index].data_type == U8:
            vals, ok, lim = tab.cols[e.expr.index].parsed(e.data_type)
            assert not lim, "a row at the program limit: not an expected-value query"
            vals = vals.copy()
            vals[~ok] = 0
            tab = tab.with_column(e.data_type, vals, ok)
            return Column(len(tab.fields) - 1), tab
        x, tab = lower(e.expr, tab)
        src = oracle_eval(tab, x)
        if src.data_type == BOOL and e.data_type != BOOL:  # true -> 1, false -> 0
            vals = np.array(src.numpy_values()).astype(bool).astype(np_dtype(e.data_type))
        elif e.data_type == BOOL and src.data_type != BOOL:  # x != 0: NaN true, -0.0 false
            vals = np.array(src.numpy_values()) != 0
        else:
            return Cast(x, e.data_type), tab
        valid = src.valid_mask()
        vals[~valid] = 0
        tab = tab.with_column(e.data_type, vals, valid)
        return Column(len(tab.fields) - 1), tab
    if isinstance(e, BinaryExpr):
        l, tab = lower(e.left, tab)
        r, tab = lower(e.right, tab)
        return BinaryExpr(l, e.op, r), tab
    return e, tab


def lower_all(exprs, tab):
    out = []
    for e in exprs:
        e, tab = lower(e, tab)
        out.append(e)
    return out, tab


def filtered(tab, pred):
    """The Selection's output: every column's selected rows, validity dropped."""
    if pred is None:
        return tab
    p, t2 = lower(pred, tab)
    n = tab.rows()
    t2 = t2.with_column(I64, np.arange(n, dtype=np.int64), np.ones(n, bool))
    keep = [i for i, f in enumerate(tab.fields) if f.data_type != U8]
    out = oracle_filter_project(t2.schema, t2.oracle_batch(), p, [Column(i) for i in keep] + [Column(len(t2.fields) - 1)],
                                FL & ~ANY)
    ids = np.array(out[-1][1].numpy_values())
    cols = []
    for i, f in enumerate(tab.fields):
        cols.append(tab.cols[i].take(ids) if f.data_type == U8 else out[keep.index(i)][1])
    return Table([Field(f.name, f.data_type, False) for f in tab.fields], cols)


def expected(tab, pred, projs):
    ps, t = lower_all(projs, filtered(tab, pred))
    return [a for _, a in oracle_filter_project(t.schema, t.oracle_batch(), None, ps, FL & ~ANY)]


def programs(tab, pred, projs, flags=FL):
    p = compile_scalar_expr(None, pred, tab.schema, flags) if pred is not None else None
    return p, [compile_scalar_expr(None, e, tab.schema, flags) for e in projs]


def device(tab, pred, projs, flags=FL, pad=0):
    p, cp = programs(tab, pred, projs, flags)
    return [a.cpu() for a in engine().filter_project(p, cp, tab.device_batch(pad), flags)]


def device_error(tab, pred, projs, flags=FL):
    with pytest.raises(ExecutionError) as e:
        device(tab, pred, projs, flags)
    return e.value.kind, e.value.message


def assert_null_slots_zero(a):
    if a.data_type == BOOL:
        assert not np.array(a.numpy_values())[~a.valid_mask()].any()
    else:
        v = np.array(a.numpy_values())
        assert not v.view("u%d" % v.dtype.itemsize)[~a.valid_mask()].any()


def cast(i, t):
    return Cast(Column(i), t)


def lt(e, v):
    return BinaryExpr(e, Operator.Lt, Literal(Float64(v)))


# ------------------------------------------------------ 1. dense projections
POOL = [s for s in CORPUS if s != LIMIT_STRING] + random_strings(600, 11, long_too=True)


def corpus_column(n, seed):
    """The corpus first (as much of it as fits), then strings of the pool;
    about 10 % nulls, which keep their bytes."""
    rng = np.random.default_rng(seed)
    head = [s for s in CORPUS if s != LIMIT_STRING][:n]
    rest = [POOL[i] for i in rng.integers(0, len(POOL), n - len(head))]
    valid = rng.random(n) >= 0.1
    if n > 200:
        valid[:len(head)] = True  # every corpus entry is parsed; nulls among the rest
    return Str(head + rest, valid)


def check_dense(n, pad):
    col = corpus_column(n, 100 + n)
    tab = Table([Field("s", U8, True)], [col])
    got = device(tab, None, [cast(0, t) for t in TARGETS], pad=pad)
    for t, g in zip(TARGETS, got):
        vals, ok, lim = col.parsed(t)
        assert not lim
        what = "%s n=%d pad=%d" % (t.name, n, pad)
        assert g.data_type == t and g.length == n, what
        assert g.null_count == int(n - ok.sum()), (what, g.null_count, int(n - ok.sum()))
        assert np.array_equal(g.valid_mask(), ok), (what, np.flatnonzero(g.valid_mask() != ok)[:5])
        gv = np.array(g.numpy_values())
        if t in FLOATS:
            gv, vals = gv.view("u%d" % t.width), vals.view("u%d" % t.width)
        bad = np.flatnonzero((gv != vals) & ok)
        assert not len(bad), (what, [(col.strings[i], gv[i], vals[i]) for i in bad[:5]])
        assert_null_slots_zero(g)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 10_000])
def test_dense_projection_of_every_target_over_the_corpus(n):
    """The wave edge, the tile edge, the tail tile, three tiles; the byte base
    at each of the 4 misalignments."""
    for pad in (0, 1, 2, 3):
        check_dense(n, pad)


# ----------------------------------------------------------- 2. filtered kernel
def number_column(n, seed, long_strings):
    """Decimal renderings of values in [0, 1e6): integers (at most 7 bytes),
    or -- long_strings -- half of them with 12 fraction digits (over 16 bytes,
    which an integer target does not parse). 10 % nulls that keep their bytes."""
    rng = np.random.default_rng(seed)
    pool_v = rng.integers(0, 10 ** 6, 1500)
    pool = [str(int(v)).encode() for v in pool_v]
    if long_strings:
        pool = [p + b".%012d" % int(f) if i % 2 else b"00000000000" + p
                for i, (p, f) in enumerate(zip(pool, rng.integers(0, 10 ** 12, 1500)))]
    idx = rng.integers(0, len(pool), n)
    return Str([pool[i] for i in idx], rng.random(n) >= 0.1), pool_v[idx]


@pytest.mark.parametrize("long_strings", [False, True], ids=["at_most_16_bytes", "over_16_bytes"])
@pytest.mark.parametrize("n", [10_000, 40_000])
def test_filtered_kernel(n, long_strings):
    """SELECT v, CAST(s AS Int64) WHERE CAST(s AS Float64) < L at about 1 / 50 /
    99 % of the non-null rows; a null s is selected (arrow's NULL < x) and its
    slot is then parsed by its raw bytes."""
    col, vals = number_column(n, 7 + n, long_strings)
    v = Array.from_numpy(I64, np.arange(n, dtype=np.int64) * 3)
    tab = Table([Field("s", U8, True), Field("v", I64, False)], [col, v])
    nulls = int(n - col.valid.sum())
    for frac in (0.01, 0.5, 0.99):
        L = float(np.quantile(vals, frac)) + 0.5
        pred, projs = lt(cast(0, F64), L), [Column(1), cast(0, I64)]
        want = expected(tab, pred, projs)
        sel = want[0].length
        assert abs((sel - nulls) / (n - nulls) - frac) < 0.02 and nulls > 0, (sel, frac)
        got = device(tab, pred, projs, pad=1)
        for g, w in zip(got, want):
            assert_same(g, w, "n=%d frac=%g" % (n, frac))
            assert g.null_count == w.null_count
        assert (want[1].null_count > 0) == long_strings  # the fraction strings are no integers
        assert_null_slots_zero(got[1])


# ------------------------------------------------------- 3. Boolean <-> numeric
def edge_numbers(t):
    if t in FLOATS:
        f = np_dtype(t)
        return np.array([0.0, -0.0, 1.0, -1.0, np.nan, -np.nan, np.inf, -np.inf, np.finfo(f).tiny, 5e-324, 0.5, 2.0 ** 40],
                        f)
    info = np.iinfo(np_dtype(t))
    return np.array([0, 1, info.min, info.max, 2, 100, 0, 7, info.max - 1, 0, 3, 1], np_dtype(t))


def bool_table(n=4097 + 12, seed=3):
    rng = np.random.default_rng(seed)
    fields = [Field("b", BOOL, True), Field("x", F64, True), Field("k", I64, False)]
    cols = [Array.from_numpy(BOOL, rng.random(n) < 0.4, rng.random(n) >= 0.2),
            Array.from_numpy(F64, rng.random(n), rng.random(n) >= 0.1), Array.from_numpy(I64, rng.integers(0, 12, n))]
    for t in NUMERIC:
        e = edge_numbers(t)
        body = rng.integers(-3, 4, n - len(e)).astype(np_dtype(t)) if t not in INTS[4:] else rng.integers(0, 4, n - len(e))
        fields.append(Field("c_" + t.name, t, True))
        cols.append(Array.from_numpy(t, np.concatenate([e, body.astype(np_dtype(t))]), rng.random(n) >= 0.15))
    return Table(fields, cols)


def test_boolean_to_and_from_every_numeric_type():
    tab = bool_table()
    n = tab.rows()
    b_vals, b_ok = np.array(tab.cols[0].numpy_values()).astype(bool), tab.cols[0].valid_mask()
    halves = [[cast(0, t) for t in NUMERIC], [cast(3 + i, BOOL) for i in range(len(NUMERIC))]]  # (16 outputs per call)
    got = device(tab, None, halves[0]) + device(tab, None, halves[1])
    for i, t in enumerate(NUMERIC):
        g = got[i]
        assert g.data_type == t and g.length == n and np.array_equal(g.valid_mask(), b_ok), t
        want = np.where(b_ok, b_vals, False).astype(np_dtype(t))
        assert np.array_equal(np.array(g.numpy_values()).view("u%d" % t.width), want.view("u%d" % t.width)), t
        g = got[len(NUMERIC) + i]
        src = tab.cols[3 + i]
        ok = src.valid_mask()
        want = (np.array(src.numpy_values()) != 0) & ok  # NaN != 0, -0.0 == 0; a null: value bit zero
        assert g.data_type == BOOL and g.length == n and np.array_equal(g.valid_mask(), ok), t
        assert np.array_equal(np.array(g.numpy_values()).astype(bool), want), t
    nan_rows = np.flatnonzero(np.isnan(edge_numbers(F64)))
    g = got[len(NUMERIC) + NUMERIC.index(F64)]
    for r in nan_rows:
        if tab.cols[3 + NUMERIC.index(F64)].valid_mask()[r]:
            assert bool(np.array(g.numpy_values())[r])
    # and through the oracle composition (the same restatement, lowered)
    for g, w in zip(got, expected(tab, None, halves[0]) + expected(tab, None, halves[1])):
        assert_same(g, w)
    # after a Selection: validity dropped, the raw slots cast
    pred = lt(Column(1), 0.5)
    for projs in halves:
        for g, w in zip(device(tab, pred, projs), expected(tab, pred, projs)):
            assert_same(g, w, "filtered")


def conditional_counts():
    return [AggregateFunction("SUM", (cast(0, DataType.Int32),), DataType.Int32),
            AggregateFunction("SUM", (Cast(BinaryExpr(Column(1), Operator.Gt, Literal(Float64(0.5))), I64),), I64),
            AggregateFunction("COUNT", (cast(0, DataType.Int32),), DataType.UInt64)]


def lower_aggs(aggs, tab):
    args, tab = lower_all([a.args[0] for a in aggs], tab)
    return [AggregateFunction(a.name, (x,), a.return_type) for a, x in zip(aggs, args)], tab


def agg_tuple(vs):
    return [(x.type, x.is_null, x.count, 0 if x.is_null else x.bits) for x in vs]


@pytest.mark.parametrize("where", [False, True])
def test_conditional_counts_ungrouped(where):
    """SUM(CAST(b AS INT)) and SUM(CAST(x > 0.5 AS BIGINT)): the conditional count of a dialect without CASE."""
    tab = bool_table()
    aggs = conditional_counts()
    pred = lt(Column(1), 0.7) if where else None
    la, lt_ = lower_aggs(aggs, filtered(tab, pred))
    ref = oracle_aggregate(lt_.schema, lt_.oracle_batch(), None, la, FLA & ~ANY)
    st = engine().agg_state([compile_expr(None, a, tab.schema, FLA) for a in aggs])
    st.add(compile_scalar_expr(None, pred, tab.schema, FLA) if where else None, tab.device_batch(), FLA)
    dev = st.finish()
    assert agg_tuple(dev) == agg_tuple(ref)
    assert ref[0].count > 100 and ref[0].bits > 100 and ref[1].bits > 100


def run_grouped(tab, pred, key, aggs, groups=None):
    ft = filtered(tab, pred)
    (lk,), t2 = lower_all([key], ft)
    la, t2 = lower_aggs(aggs, t2)
    rk, rv, _ = oracle_aggregate_grouped_multi(t2.schema, t2.oracle_batch(), None, [lk], la, FLA & ~ANY)
    st = engine().grouped_agg_state([compile_scalar_expr(None, key, tab.schema, FLA)],
                                    [compile_expr(None, a, tab.schema, FLA) for a in aggs])
    st.add(compile_scalar_expr(None, pred, tab.schema, FLA) if pred is not None else None, tab.device_batch(), FLA)
    dk, dv = st.finish()
    assert len(dk) == len(rk), (len(dk), len(rk))
    if groups is not None:
        assert len(rk) == groups
    for g in range(len(rk)):
        assert agg_tuple(dk[g]) == agg_tuple(rk[g]), g
        assert agg_tuple(dv[g]) == agg_tuple(rv[g]), g
    return rk


def test_conditional_counts_grouped():
    run_grouped(bool_table(), None, Column(2), conditional_counts(), 12)
    run_grouped(bool_table(), lt(Column(1), 0.7), Column(2), conditional_counts(), 12)


# ------------------------------------------------- 4. aggregate arguments, keys
def key_table(n, seed, wide):
    """s: integers in a narrow range (the key window) or spread over 2^40 (the
    hash table), a few unparsable strings (null keys) and null rows; w Float64."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 20, n) if not wide else rng.choice(rng.integers(-(1 << 40), 1 << 40, 37), n)
    strings = [str(int(k)).encode() for k in keys]
    for i in rng.integers(0, n, n // 50):
        strings[i] = [b"x", b"", b"1.5", b"12 "][i % 4]
    tab = Table([Field("s", U8, True), Field("w", F64, False), Field("d", U8, False)],
                [Str(strings, rng.random(n) >= 0.1), Array.from_numpy(F64, rng.random(n)),
                 Str([repr(float(x)).encode() for x in rng.standard_normal(n) * 1e3])])
    return tab


def test_sum_of_a_parsed_column():
    tab = key_table(6000, 5, False)
    aggs = [AggregateFunction("SUM", (cast(2, F64),), F64), AggregateFunction("SUM", (cast(0, I64),), I64),
            AggregateFunction("COUNT", (cast(0, I64),), DataType.UInt64), AggregateFunction("MIN", (cast(2, F64),), F64)]
    for pred in (None, lt(Column(1), 0.6), lt(cast(2, F64), 0.0)):
        la, t2 = lower_aggs(aggs, filtered(tab, pred))
        ref = oracle_aggregate(t2.schema, t2.oracle_batch(), None, la, FLA & ~ANY)
        st = engine().agg_state([compile_expr(None, a, tab.schema, FLA) for a in aggs])
        st.add(compile_scalar_expr(None, pred, tab.schema, FLA) if pred is not None else None, tab.device_batch(), FLA)
        assert agg_tuple(st.finish()) == agg_tuple(ref), repr(pred)
        assert ref[2].bits > 1000


@pytest.mark.parametrize("wide", [False, True], ids=["window", "hash_table"])
def test_group_by_a_parsed_key(wide):
    """GROUP BY CAST(s AS BIGINT): the null key comes from null rows and from
    strings that do not parse."""
    tab = key_table(6000, 9, wide)
    aggs = [AggregateFunction("SUM", (cast(2, F64),), F64), AggregateFunction("COUNT", (Column(1),), DataType.UInt64)]
    rk = run_grouped(tab, None, cast(0, I64), aggs, (37 if wide else 20) + 1)
    assert any(k[0].is_null for k in rk)
    run_grouped(tab, lt(Column(1), 0.5), cast(0, I64), aggs)


def test_order_by_a_parsed_key():
    n = 3000
    rng = np.random.default_rng(23)
    v = rng.integers(-10 ** 9, 10 ** 9, n)
    strings = [str(int(x)).encode() for x in v]
    for i in (5, 77, 1500):
        strings[i] = b"9e9"  # no integer: a null key, greater than every value, first under DESC
    s = Schema([Field("s", U8, False), Field("i", I64, False)])
    cols = [Col(U8, strings), Col(I64, np.arange(n))]
    tab = Table(s.fields, [Str(strings), Array.from_numpy(I64, np.arange(n))])
    flags = FL | _abi.DFMI_FLAG_EXT_SORT | _abi.DFMI_FLAG_EXT_UTF8_COMPARE
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(s, [tab.device_batch()]))
    (rb,) = pull_all(ctx.sql("SELECT s, i FROM t ORDER BY CAST(s AS BIGINT) DESC LIMIT 5"))
    kv, kok, _ = Str(strings).parsed(I64)
    check(rb.columns, cols, expected_order(cols + [Col(I64, kv, kok)], [(2, False)], 5))


# ------------------------------------------------------------ 5. batch forms
FORMS_SQL = "SELECT v, CAST(s AS BIGINT), CAST(s AS DOUBLE), CAST(b AS INT) FROM t WHERE CAST(s AS DOUBLE) < 500000"


def forms_table(n, seed):
    col, _ = number_column(n, seed, True)
    rng = np.random.default_rng(seed)
    return Table([Field("s", U8, True), Field("v", I64, False), Field("b", BOOL, True)],
                 [col, Array.from_numpy(I64, np.arange(n, dtype=np.int64)),
                  Array.from_numpy(BOOL, rng.random(n) < 0.5, rng.random(n) >= 0.2)])


def forms_query(tab):
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(tab.schema, []))
    plan = SqlToRel(ctx).sql_to_rel(FORMS_SQL)
    return plan.input.expr, plan.expr


def split_table(tab, sizes):
    out, lo = [], 0
    for sz in sizes:
        cols = []
        for c in tab.cols:
            if isinstance(c, Str):
                cols.append(Str(c.strings[lo:lo + sz], c.valid[lo:lo + sz]))
            else:
                m = c.valid_mask()[lo:lo + sz]
                cols.append(Array.from_numpy(c.data_type, np.array(c.numpy_values())[lo:lo + sz], None if m.all() else m))
        out.append(Table(tab.fields, cols))
        lo += sz
    return out


def test_every_batch_form_gives_the_same_bits():
    sizes = [1024] * 3 + [0, 777]
    tab = forms_table(sum(sizes), 41)
    pred, projs = forms_query(tab)
    parts = split_table(tab, sizes)
    want = [expected(t, pred, projs) for t in parts]
    whole = expected(tab, pred, projs)
    assert 500 < whole[0].length < sum(sizes) - 500 and whole[1].null_count > 0
    p, cp = programs(tab, pred, projs)
    # one device batch
    for g, w in zip(engine().filter_project(p, cp, tab.device_batch(3), FL), whole):
        assert_same(g.cpu(), w, "device")
    # coalesced device batches of 1024 rows
    results, err = engine().filter_project_batches(p, cp, [t.device_batch() for t in parts], FL)
    assert err is None and len(results) == len(sizes)
    for res, w in zip(results, want):
        for g, x in zip(res, w):
            assert_same(g.cpu(), x, "device batches")
    # one host batch; many host batches in one call
    for g, w in zip(engine().filter_project_host(p, cp, tab.host_batch(), FL), whole):
        assert_same(g, w, "host batch")
    hres, herr = engine().filter_project_host_batches(p, cp, [t.host_batch() for t in parts], FL)
    assert herr is None and len(hres) == len(sizes)
    for res, w in zip(hres, want):
        for g, x in zip(res.materialize(), w):
            assert_same(g, x, "host batches")
    # a sliced batch: rows [1000, 3000) of the same buffers
    lo, ln = 1000, 2000
    db = tab.device_batch(2)
    sliced = RecordBatch(tab.schema, [c.slice(lo, ln) for c in db.columns])
    cut = split_table(tab, [lo, ln])[1]
    for g, w in zip(engine().filter_project(p, cp, sliced, FL), expected(cut, pred, projs)):
        assert_same(g.cpu(), w, "sliced")


def test_chunked_host_batch(monkeypatch):
    tab = forms_table(70_001, 43)  # (chunks are pipelined only past 65,536 rows)
    pred, projs = forms_query(tab)
    want = expected(tab, pred, projs)
    p, cp = programs(tab, pred, projs)
    monkeypatch.setenv("DFMI_HOST_CHUNK_ROWS", "8192")
    for g, w in zip(engine().filter_project_host(p, cp, tab.host_batch(), FL), want):
        assert_same(g, w, "chunked host batch")


def test_ctx_sql_and_the_serde_worker():
    tab = forms_table(5000, 47)
    pred, projs = forms_query(tab)
    want = expected(tab, pred, projs)
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(tab.schema, [tab.device_batch()]))
    assert repr(SqlToRel(ctx).sql_to_rel(FORMS_SQL).expr[1]) == "CAST(#0 AS Int64)"
    (rb,) = pull_all(ctx.sql(FORMS_SQL))
    for g, w in zip(rb.columns, want):
        assert_same(g.cpu(), w, "ctx.sql")
    ctx0 = ExecutionContext(flags=FL & ~ANY)
    ctx0.register_datasource("t", MemoryDataSource(tab.schema, [tab.device_batch()]))
    with pytest.raises(ExecutionError) as e:
        pull_all(ctx0.sql(FORMS_SQL))
    assert (e.value.kind, e.value.message) == (NOT_IMPL, "CAST from Utf8 to Float64")
    # the worker: the plan as JSON in, an Arrow stream out
    ctxw = ExecutionContext(flags=FL)
    ctxw.register_datasource("t", MemoryDataSource(tab.schema, [tab.host_batch()]))
    plan = SqlToRel(ctxw).sql_to_rel(FORMS_SQL)
    t = pa.ipc.open_stream(serde.run_physical_plan(ctxw, serde.to_json(serde.Interactive(plan)))).read_all()
    assert t.num_rows == want[0].length
    for j, w in enumerate(want):
        got = t.column(j).combine_chunks()
        ok = w.valid_mask()
        assert got.null_count == w.null_count and np.array_equal(np.array(got.is_valid()), ok), j
        gv = got.fill_null(0).to_numpy(zero_copy_only=False)
        wv = np.array(w.numpy_values())
        assert np.array_equal(gv[ok].view("u%d" % wv.dtype.itemsize), wv[ok].view("u%d" % wv.dtype.itemsize)), j


# --------------------------------------------------------- 6. the program limit
def limit_table(n=3000, at=2100, null_at=700, w_fill=1.0):
    rng = np.random.default_rng(3)
    strings = [repr(float(x)).encode() for x in rng.random(n) * 100]
    strings[at] = LIMIT_STRING
    strings[null_at] = LIMIT_STRING  # a null row: raises nothing
    valid = np.ones(n, bool)
    valid[null_at] = False
    w = np.full(n, w_fill)
    return Table([Field("s", U8, True), Field("w", F64, False), Field("z", F64, False)],
                 [Str(strings, valid), Array.from_numpy(F64, w), Array.from_numpy(F64, rng.random(n))])


def test_the_limit_row_raises_the_defined_error():
    tab = limit_table()
    for t in FLOATS[1:]:
        err = (NOT_IMPL, limit_message(t))
        assert device_error(tab, None, [cast(0, t)]) == err
        assert device_error(tab, lt(cast(0, t), 50.0), [Column(1)]) == err
        assert device_error(tab, lt(Column(1), 5.0), [cast(0, t)]) == err
    # Float32: both brackets round to 2^53, no error; the integer targets: a null row
    got = device(tab, None, [cast(0, DataType.Float32), cast(0, I64), cast(0, DataType.UInt8)])
    assert np.array(got[0].numpy_values())[2100] == np.float32(2.0 ** 53) and got[0].valid_mask()[2100]
    assert not got[0].valid_mask()[700]
    assert not got[1].valid_mask()[2100] and not got[2].valid_mask()[2100]
    # not selected: nothing raised (z < 0 selects no row; w = 1 is not < 0.5)
    got = device(tab, lt(Column(1), 0.5), [cast(0, F64)])
    assert got[0].length == 0


def test_the_limit_reports_its_row_and_loses_to_an_earlier_ordinal():
    # two limit rows: the first by row wins (the error key names ordinal, then row)
    two = limit_table()
    two.cols[0].strings[900] = LIMIT_STRING
    p, cp = programs(two, None, [cast(0, F64)])
    with pytest.raises(ExecutionError) as e:
        engine().filter_project(p, cp, two.device_batch(), FL)
    assert (e.value.kind, e.value.message) == (NOT_IMPL, limit_message(F64))
    assert (e.value.order_key >> 4) & ((1 << 40) - 1) == 900 and e.value.order_key >> 44 == 3  # (2 + the node's postfix position)
    # a DivideByZero at a lower ordinal in the same batch wins, whatever its row
    zero = limit_table(w_fill=0.0)
    div = BinaryExpr(Column(2), Operator.Divide, Column(1))  # ordinals before the second projection's
    assert device_error(zero, None, [div, cast(0, F64)]) == ("ArrowError(DivideByZero)", "DivideByZero")
    # ... and loses where the cast comes first
    kind, msg = device_error(zero, None, [cast(0, F64), div])
    assert (kind, msg) == (NOT_IMPL, limit_message(F64))


def test_the_limit_in_coalesced_batches_names_the_batch_that_raised_it():
    sizes = [1024, 1024, 952]
    tab = limit_table(n=3000, at=2100)  # row 2100: batch 2, its row 52
    parts = split_table(tab, sizes)
    p, cp = programs(tab, None, [Column(1), cast(0, F64)])
    results, err = engine().filter_project_batches(p, cp, [t.device_batch() for t in parts], FL)
    assert err is not None and (err.kind, err.message) == (NOT_IMPL, limit_message(F64))
    assert err.failed_batch == 2 and len(results) == 2
    for res, t in zip(results, parts):
        for g, w in zip(res, expected(t, None, [Column(1), cast(0, F64)])):
            assert_same(g.cpu(), w)
    hres, herr = engine().filter_project_host_batches(p, cp, [t.host_batch() for t in parts], FL)
    assert herr is not None and (herr.kind, herr.message) == (NOT_IMPL, limit_message(F64)) and herr.failed_batch == 2
