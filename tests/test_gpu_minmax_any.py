"""MIN / MAX over a Boolean or Utf8 argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY)
on the device. First the Boolean extremes (the Utf8 ones follow further down
under their own heading), on every path a numeric MIN / MAX takes -- ungrouped states, the window
kernel, the hash table's scattered and bucketed passes, the host merge, the
host and device finishes and emission, coalesced device and host batches,
partials and their merges, the world-size-1 shard finishes, ctx.sql and the
reference's own aggregate fixtures.

The oracle executes no Boolean extreme and is left as it is. The expected
extreme is Python's min / max over the bools of the rows that count (the valid
slots; after a Selection every selected slot with its raw bit); everything
around it -- group keys and their order, row counts, the extreme's count and
null flag, the other aggregates bit for bit -- is the oracle's, called with
COUNT(e) in the extreme's place."""
import functools

import numpy as np
import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, RecordBatch
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.aggregate import AggregateRelation
from datafusion_amd.execution.engine import ShardComm, engine, merge_agg_partials, merge_grouped_partials
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator
from oracle_ffi import oracle_aggregate, oracle_aggregate_grouped_multi
from test_aggregate_cpu import agg, wild_doubles
from test_gpu_avg import Table, _bucketed_batches, _tuple, exprs, run_state, same

pytestmark = pytest.mark.gpu

AGG = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_GATHER_ALL
FL = AGG | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY
BOOL = int(DataType.Boolean)


def is_extreme(t: Table, f: str, c: int) -> bool:
    return f.upper() in ("MIN", "MAX") and t.types[c] == DataType.Boolean


def count_in_place(t: Table, aggs):
    return [("COUNT", c) if is_extreme(t, f, c) else (f, c) for f, c in aggs]


def check_values(t: Table, aggs, got, ref, rows, dropped_validity):
    """One group's (or the ungrouped) values: a Boolean extreme's count is the
    oracle's COUNT in its place, its value Python's min / max over the rows
    that count; every other aggregate is the oracle's."""
    for j, ((f, c), d, r) in enumerate(zip(aggs, got, ref)):
        if not is_extreme(t, f, c):
            assert _tuple(d) == _tuple(r), (j, f)
            continue
        counted = [bool(t.values[c][i]) for i in rows if dropped_validity or t.valid[c][i]]
        assert len(counted) == int(r.bits), (j, f)
        want = (min if f.upper() == "MIN" else max)(counted) if counted else None
        assert (int(d.type), int(d.count)) == (BOOL, len(counted)), (j, f)
        if want is None:
            assert d.is_null, (j, f)
        else:
            assert not d.is_null and int(d.bits) == int(want), (j, f, int(d.bits), want)


def check(t: Table, pred, mask, keys, aggs, got):
    sel = np.arange(t.n) if mask is None else np.nonzero(mask)[0]
    dropped = mask is not None  # FilterRelation::next copies raw slots: the filtered batch has no validity
    ref_aggs = exprs(t, count_in_place(t, aggs))
    if keys is None:
        ref = oracle_aggregate(t.schema, t.batch, pred, ref_aggs, AGG)
        check_values(t, aggs, got, ref, list(sel), dropped)
        return
    rk, rv, rs = oracle_aggregate_grouped_multi(t.schema, t.batch, pred, [Column(k) for k in keys], ref_aggs, AGG)
    dk, dv, strs = got
    assert len(dk) == len(rk)
    groups = {}
    for i in sel:  # (a predicate's cases group by keys without nulls: a filtered null key is a raw slot)
        groups.setdefault(tuple(t.key_of(k, i) for k in keys), []).append(i)
    assert len(groups) == len(rk)
    for g in range(len(rk)):
        assert [(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in dk[g]] == \
            [(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in rk[g]], g
        key = []
        for q, k in enumerate(keys):
            if rs[q] is not None:
                assert strs[q][g] == rs[q][g], (g, q)
                key.append(rs[q][g])
            else:
                key.append(None if rk[g][q].is_null else int(rk[g][q].bits))
        check_values(t, aggs, dv[g], rv[g], groups[tuple(key)], dropped)


@functools.lru_cache(maxsize=None)
def table(nkeys: int = 300, n: int = 5000) -> Table:
    """n rows (5,000: one full 4,096-row tile plus a tail): Boolean arguments
    with 15% nulls (`b` mostly true, `c` mostly false, every value of some keys
    null or all equal), a Float64 argument, a predicate column, an Int8 key of
    5 values, a Boolean key, ~nkeys wide Int64 keys, a Utf8 key, and a wide
    Int64 key without nulls."""
    rng = np.random.default_rng(91 + nkeys + n)
    k = rng.integers(0, nkeys, n)
    b, c = rng.random(n) < 0.9, rng.random(n) < 0.1
    vb, vc = rng.random(n) >= 0.15, rng.random(n) >= 0.15
    vb[k % 17 == 3] = False   # a null extreme
    b[k % 13 == 2] = True     # MIN = true
    c[k % 11 == 4] = False    # MAX = false
    words = [bytes(rng.integers(97, 123, int(ln)).astype(np.uint8)) for ln in rng.integers(0, 30, 40)]
    return Table([("b", DataType.Boolean, b, vb), ("c", DataType.Boolean, c, vc),
                  ("x", DataType.Float64, wild_doubles(rng, n), rng.random(n) >= 0.1),
                  ("p", DataType.Float64, rng.random(n), None),
                  ("k8", DataType.Int8, rng.integers(-2, 3, n).astype(np.int8), rng.random(n) >= 0.05),
                  ("kb", DataType.Boolean, rng.random(n) < 0.5, rng.random(n) >= 0.05),
                  ("k", DataType.Int64, k * 1_000_003_000 - 7_000_000_000_000, rng.random(n) >= 0.02),
                  ("s", DataType.Utf8, [None if rng.random() < 0.02 else words[i] for i in k % 40], None),
                  ("kn", DataType.Int64, k * 1_000_003_000 - 7_000_000_000_000, None)])


B, C_, X, P, K8, KB, K, S, KN = range(9)
AGGS = [("MIN", B), ("MAX", B), ("SUM", X), ("min", C_), ("COUNT", B), ("max", C_), ("MIN", X)]
PRED = BinaryExpr(Column(P), Operator.Lt, Literal(Float64(0.6)))


# ------------------------------------------------------------------ ungrouped
@pytest.mark.parametrize("batch_rows", [0, 1024])
def test_ungrouped(batch_rows):
    t = table()
    check(t, None, None, None, AGGS, run_state(t, None, None, AGGS, batch_rows, flags=FL))
    check(t, PRED, t.values[P] < 0.6, None, AGGS, run_state(t, PRED, None, AGGS, batch_rows, flags=FL))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ungrouped_small_row_counts(n):
    t = table(7, n)
    check(t, None, None, None, AGGS, run_state(t, None, None, AGGS, flags=FL))
    check(t, None, None, [K], AGGS, run_state(t, None, [K], AGGS, flags=FL))


def test_ungrouped_nothing_counts_and_raw_null_slots():
    t = table()
    none = BinaryExpr(Column(P), Operator.Lt, Literal(Float64(-1.0)))
    got = run_state(t, none, None, AGGS, flags=FL)
    check(t, none, np.zeros(t.n, bool), None, AGGS, got)
    assert got[0].is_null and got[1].is_null and (int(got[0].type), int(got[0].count)) == (BOOL, 0)
    # every slot null: null without a predicate; with one the raw bits count (true in a null slot)
    h = Table([("b", DataType.Boolean, np.array([False, True, False]), np.zeros(3, bool)),
               ("p", DataType.Float64, np.array([0.1, 0.2, 0.3]), None)])
    two = [("MIN", 0), ("MAX", 0)]
    got = run_state(h, None, None, two, flags=FL)
    assert [(int(v.is_null), int(v.count)) for v in got] == [(1, 0), (1, 0)]
    allp = BinaryExpr(Column(1), Operator.Lt, Literal(Float64(1.0)))
    got = run_state(h, allp, None, two, flags=FL)
    check(h, allp, np.ones(3, bool), None, two, got)
    assert [(int(v.is_null), int(v.count), int(v.bits)) for v in got] == [(0, 3, 0), (0, 3, 1)]


def test_expression_argument():
    """MIN / MAX of a comparison (a Boolean expression, not a column)."""
    t = table()
    s = t.schema
    e = BinaryExpr(Column(X), Operator.Lt, Literal(Float64(0.0)))
    cs = [compile_expr(None, agg(f, e, s), s, FL) for f in ("MIN", "MAX", "COUNT")]
    st = engine().agg_state(cs)
    st.add(None, t.batch.to(engine().device), FL)
    mn, mx, cnt = st.finish()
    # (a comparison is never null: a null operand is less than every value, arrow's cmp_opt)
    neg = [bool(v < 0) or not ok for v, ok in zip(t.values[X], t.valid[X])]
    (ref,) = oracle_aggregate(s, t.batch, None, [agg("COUNT", e, s)], AGG)
    assert (int(mn.type), int(mn.bits), int(mx.bits)) == (BOOL, int(min(neg)), int(max(neg)))
    assert int(mn.count) == int(mx.count) == int(cnt.bits) == int(ref.bits) == len(neg)


# ------------------------------------------------------- window and hash table
@pytest.mark.parametrize("batch_rows", [0, 1024])
def test_window_kernel(batch_rows):
    """One Int8 key of 5 values and the null key, and a Boolean key: the fused grouped kernel."""
    t = table()
    got = run_state(t, None, [K8], AGGS, batch_rows, flags=FL)
    assert len(got[0]) == 6
    check(t, None, None, [K8], AGGS, got)
    got = run_state(t, None, [KB], AGGS, batch_rows, flags=FL)
    assert len(got[0]) == 3
    check(t, None, None, [KB], AGGS, got)


@pytest.mark.parametrize("buckets", ["1", "0"])
@pytest.mark.parametrize("batch_rows", [0, 1_001])
def test_hash_table_few_keys(monkeypatch, buckets, batch_rows):
    """~300 wide Int64 keys: the bucketed passes (forced at this size) and the
    per-row accumulate pass; a predicate over the key without nulls."""
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_GROUP_BUCKETS", buckets)
    t = table()
    before = _bucketed_batches()
    got = run_state(t, None, [K], AGGS, batch_rows, flags=FL)
    assert (_bucketed_batches() > before) == (buckets == "1")
    assert len(got[0]) == 301 and any(v[0].is_null for v in got[1])
    assert {int(v[0].bits) for v in got[1] if not v[0].is_null} == {0, 1}
    check(t, None, None, [K], AGGS, got)
    check(t, PRED, t.values[P] < 0.6, [KN], AGGS, run_state(t, PRED, [KN], AGGS, batch_rows, flags=FL))


@pytest.mark.parametrize("emit", ["0", "1"])
def test_many_keys_growth_and_device_emission(monkeypatch, emit):
    """~4,000 keys in 5,000 rows: table records grow (1,024 at first), and with
    DFMI_GROUP_DEVICE_EMIT=1 k_group_emit finishes the Boolean extreme."""
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_GROUP_DEVICE_EMIT", emit)
    t = table(15_000)
    got = run_state(t, None, [KN], AGGS, 1_001, flags=FL)
    assert len(got[0]) > 2_500
    check(t, None, None, [KN], AGGS, got)


def test_utf8_key_key_pair_and_forced_paths(monkeypatch):
    """A Utf8 key and an (Int64, Utf8) pair; then the same state through the
    host finish, the host merge and a 3-bit hash (rows collide: the host
    merges them) -- the same result."""
    t = table()
    check(t, None, None, [S], AGGS, run_state(t, None, [S], AGGS, 1_001, flags=FL))
    dev = run_state(t, None, [K, S], AGGS, 1_001, flags=FL)
    check(t, None, None, [K, S], AGGS, dev)
    monkeypatch.setenv("DFMI_DIAG", "1")
    for knob, value in (("DFMI_GROUP_HOST_FINISH", "1"), ("DFMI_GROUP_HOST", "1"), ("DFMI_GROUP_HASH_BITS", "3")):
        monkeypatch.setenv(knob, value)
        same(dev, run_state(t, None, [K, S], AGGS, 1_001, flags=FL))
        monkeypatch.delenv(knob)


# ----------------------------------------------------- batch forms and partials
@pytest.mark.parametrize("host", [False, True], ids=["device_batches", "host_batches"])
def test_coalesced_batches_equal_one_call_per_batch(host):
    t = table()
    for keys in (None, [K8], [K]):
        one = run_state(t, None, keys, AGGS, 257, flags=FL)
        same(one, run_state(t, None, keys, AGGS, 257, many=True, host=host, flags=FL))
        check(t, None, None, keys, AGGS, one)


def test_sliced_input_and_finish_then_more():
    """A sliced input array (arrow offsets), and more batches after a finish."""
    t = table()
    for keys in (None, [K]):
        s = t.schema
        cs = [compile_expr(None, a, s, FL) for a in exprs(t, AGGS)]
        eng = engine()
        st = eng.agg_state(cs) if keys is None else eng.grouped_agg_state(
            [compile_scalar_expr(None, Column(k), s, FL) for k in keys], cs)
        dev = t.batch.to(eng.device)
        from test_gpu_aggregate import slice_batch
        st.add(None, slice_batch(dev, 0, 1_003), FL)
        first = st.finish()
        st.add(None, slice_batch(dev, 1_003, t.n - 1_003), FL)
        out = st.finish()
        got = out if keys is None else (out[0], out[1], [None])
        check(t, None, None, keys, AGGS, got)
        head = t.rows(0, 1_003)
        check(head, None, None, keys, AGGS, first if keys is None else (first[0], first[1], [None]))
        st.reset()
        st.add(None, slice_batch(dev, 0, 1_003), FL)
        again = st.finish()
        same(first if keys is None else (first[0], first[1], None), again if keys is None else (again[0], again[1], None))


def test_merged_partials_equal_one_state():
    """A Boolean extreme's partial is an integer MIN / MAX partial over 0 / 1."""
    def partial(st, cs):
        return cs, st.partial()
    t = table()
    parts = []
    for r0, r1 in ((0, 2048), (2048, t.n)):
        cs, p = run_state(t.rows(r0, r1), None, None, AGGS, flags=FL, finish=partial)
        parts.append(p)
    whole = run_state(t, None, None, AGGS, flags=FL)
    same(whole, merge_agg_partials(cs, parts))
    check(t, None, None, None, AGGS, whole)
    whole = run_state(t, None, [K], AGGS, flags=FL)
    parts = []
    for r0, r1 in ((0, 2_000), (2_000, t.n)):
        cs, p = run_state(t.rows(r0, r1), None, [K], AGGS, flags=FL, finish=partial)
        parts.append(p)
    mk, mv = merge_grouped_partials(cs, parts, 1, True)
    same((whole[0], whole[1], None), (mk, mv, None))


def test_world_size_one_shard_finishes():
    comm = ShardComm(engine(), 1, 0, ShardComm.unique_id())
    t = table()
    same(run_state(t, None, None, AGGS, flags=FL),
         run_state(t, None, None, AGGS, flags=FL, finish=lambda st, cs: comm.agg_finish(st)))
    whole = run_state(t, None, [K], AGGS, flags=FL)
    mk, mv = run_state(t, None, [K], AGGS, flags=FL, finish=lambda st, cs: comm.agg_finish_grouped(st))
    same((whole[0], whole[1], None), (mk, mv, None))


# ------------------------------------------------------ fixtures, SQL, relation
@pytest.mark.parametrize("batch_rows", [0, 64])
def test_reference_fixture_cells(batch_rows):
    """csv_aggregate_all_types.csv cells 2 and 3: MIN(c0), MAX(c0) of
    all_types_flat.csv, whole and as 64-row batches, through ctx.sql."""
    from golden_cases import all_types_typed, expected_rows, load_batch
    from test_gpu_aggregate import slice_batch
    schema = all_types_typed()
    batch = load_batch(schema, "all_types_flat.csv", has_header=True)
    (row,) = expected_rows("csv_aggregate_all_types.csv")
    assert row[2:4] == ["false", "true"]
    dev = batch.to(engine().device)
    step = batch_rows or batch.num_rows()
    batches = [slice_batch(dev, r0, min(step, batch.num_rows() - r0)) for r0 in range(0, batch.num_rows(), step)]
    ctx = ExecutionContext(flags=_abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY)
    ctx.register_datasource("t", MemoryDataSource(schema, batches))
    out = ctx.sql("SELECT MIN(c0), MAX(c0), COUNT(c0) FROM t").next()
    assert [f.data_type for f in out.schema.fields] == [DataType.Boolean, DataType.Boolean, DataType.UInt64]
    c0 = batch.columns[0].to_pylist()
    assert [c.to_pylist() for c in out.columns] == [[min(c0)], [max(c0)], [len(c0)]]
    assert [str(c.to_pylist()[0]).lower() for c in out.columns[:2]] == row[2:4]


def test_sql_group_by_relation_and_flagless_error():
    t = table()
    fl = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY
    dev = t.batch.to(engine().device)
    from test_gpu_aggregate import slice_batch
    batches = [slice_batch(dev, r0, min(64, t.n - r0)) for r0 in range(0, t.n, 64)]
    want = {}
    for i in range(t.n):
        if t.valid[B][i]:
            want.setdefault(t.key_of(K8, i), []).append(bool(t.values[B][i]))
    for coalesce in (1, 256):
        ctx = ExecutionContext(flags=fl)
        ctx.register_datasource("t", MemoryDataSource(t.schema, list(batches)))
        rel = ctx.sql("SELECT k8, MIN(b), MAX(b) FROM t GROUP BY k8")
        assert isinstance(rel, AggregateRelation)
        rel.coalesce = coalesce
        (rb,) = list(rel)
        keys = rb.columns[0].to_pylist()
        assert keys == [-2, -1, 0, 1, 2, None]
        ext = lambda k: None if k is None else k & (2 ** 64 - 1)  # noqa: E731
        assert rb.columns[1].to_pylist() == [min(want[ext(k)]) for k in keys]
        assert rb.columns[2].to_pylist() == [max(want[ext(k)]) for k in keys]
    old = ExecutionContext(flags=_abi.DFMI_FLAG_EXT_AGGREGATE)
    old.register_datasource("t", MemoryDataSource(t.schema, list(batches)))
    with pytest.raises(ExecutionError) as ei:
        old.sql("SELECT MIN(b) FROM t").next()
    assert (ei.value.kind, ei.value.message) == ("NotImplemented", "aggregate over Boolean")


# ============================================================ Utf8 MIN / MAX
# The same flag accepts MIN / MAX over a Utf8 argument: bytewise order (the
# GROUP BY / ORDER BY / DFMI_FLAG_EXT_UTF8_ORDER one). dfmi_agg_value carries
# type Utf8, is_null, count and bits = the value's byte length; the bytes come
# from dfmi_agg_state_value_bytes (value_strings). Expected extremes: Python's
# min / max over the bytes of the rows that count; the rest from the oracle
# with COUNT(e) in the extreme's place.
UTF8 = int(DataType.Utf8)
SFL = FL | _abi.DFMI_FLAG_EXT_UTF8_COMPARE


def is_str_extreme(t: Table, f: str, c: int) -> bool:
    return f.upper() in ("MIN", "MAX") and t.types[c] == DataType.Utf8


def any_in_place(t: Table, aggs):
    return [("COUNT", c) if is_extreme(t, f, c) or is_str_extreme(t, f, c) else (f, c) for f, c in aggs]


def with_raw_nulls(t: Table, c: int, valid) -> Table:
    """Column c (Utf8, every entry bytes) with `valid` as its validity: a null slot keeps its bytes."""
    a = t.batch.columns[c]
    valid = np.asarray(valid, bool)
    nulls = int(t.n - valid.sum())
    from datafusion_amd.arrow import _bytes_tensor, pack_bits
    cols = list(t.batch.columns)
    cols[c] = Array(DataType.Utf8, t.n, a.values, _bytes_tensor(pack_bits(valid)) if nulls else None, a.offsets, nulls)
    t.batch = RecordBatch(t.schema, cols)
    t.valid[c] = valid
    return t


def collect(t: Table, keys, aggs):
    """run_state's finish: (values or (keys, values, key strings), {j: value strings})."""
    def fin(st, cs):
        out = st.finish()
        vs = {j: st.value_strings(j) for j, (f, c) in enumerate(aggs) if is_str_extreme(t, f, c)}
        if keys is None:
            return out, vs
        dk, dv = out
        return (dk, dv, [st.key_strings(q) if t.types[k] == DataType.Utf8 else None for q, k in enumerate(keys)]), vs
    return fin


def srun(t: Table, pred, keys, aggs, batch_rows=0, many=False, host=False):
    return run_state(t, pred, keys, aggs, batch_rows, many, host, flags=SFL, finish=collect(t, keys, aggs))


def scheck_values(t, aggs, got, ref, strings, g, rows, dropped):
    for j, ((f, c), d, r) in enumerate(zip(aggs, got, ref)):
        if is_extreme(t, f, c):
            check_values(t, [aggs[j]], [d], [r], rows, dropped)
        elif is_str_extreme(t, f, c):
            counted = [t.values[c][i] or b"" for i in rows if dropped or t.valid[c][i]]
            assert len(counted) == int(r.bits), (j, f)
            want = (min if f.upper() == "MIN" else max)(counted) if counted else None
            assert (int(d.type), int(d.count), int(d.is_null)) == (UTF8, len(counted), int(want is None)), (j, f, g)
            assert strings[j][g] == want, (j, f, g, strings[j][g], want)
            assert int(d.bits) == (0 if want is None else len(want)), (j, f, g)
        else:
            assert _tuple(d) == _tuple(r), (j, f)


def scheck(t: Table, pred, mask, keys, aggs, result):
    got, vs = result
    sel = np.arange(t.n) if mask is None else np.nonzero(mask)[0]
    dropped = mask is not None
    ref_aggs = exprs(t, any_in_place(t, aggs))
    if keys is None:
        ref = oracle_aggregate(t.schema, t.batch, pred, ref_aggs, SFL)
        scheck_values(t, aggs, got, ref, vs, 0, list(sel), dropped)
        return
    rk, rv, rs = oracle_aggregate_grouped_multi(t.schema, t.batch, pred, [Column(k) for k in keys], ref_aggs, SFL)
    dk, dv, strs = got
    assert len(dk) == len(rk)
    groups = {}
    for i in sel:
        groups.setdefault(tuple(t.key_of(k, i) for k in keys), []).append(i)
    assert len(groups) == len(rk)
    for g in range(len(rk)):
        assert [(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in dk[g]] == \
            [(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in rk[g]], g
        key = []
        for q, k in enumerate(keys):
            if rs[q] is not None:
                assert strs[q][g] == rs[q][g], (g, q)
                key.append(rs[q][g])
            else:
                key.append(None if rk[g][q].is_null else int(rk[g][q].bits))
        scheck_values(t, aggs, dv[g], rv[g], vs, g, groups[tuple(key)], dropped)


def ssame(a, b):
    same(a[0], b[0])
    assert a[1] == b[1]


# ---------------------------------------------------------------- hand-built
HAND = [b"", b"a", b"a\0", b"a\x7f", b"a\x80", b"\xff", b"aaaaaaaa", b"aaaaaaaa\0", b"aaaaaaaab",
        b"b" * 7, b"b" * 8, b"b" * 9, b"b" * 15, b"b" * 16, b"b" * 17, b"c" * 299 + b"x", b"c" * 299 + b"y"]


def hand_table() -> Table:
    """Three groups (and their union, ungrouped). Group 0: every hand-built
    string once and its winners twice more; group 1: only strings sharing an
    8-byte prefix, then the two 300-byte strings; group 2: a null beside an
    empty string. Group 3: all null. `p` selects everything but the winners of
    group 0, or nothing."""
    s0 = HAND + [b"", b"", b"\xff", b"\xff"]
    s1 = [b"aaaaaaaa\0", b"aaaaaaaab", b"aaaaaaaa", b"aaaaaaaab", b"aaaaaaaa"]
    s2 = [None, b"", None]
    s3 = [None, None]
    s = s0 + s1 + s2 + s3
    k = [0] * len(s0) + [1] * len(s1) + [2] * len(s2) + [3] * len(s3)
    p = [0.0 if x in (b"", b"\xff") else 0.5 for x in s0] + [0.5] * (len(s1) + len(s2) + len(s3))
    return Table([("k", DataType.Int64, np.array(k), None), ("s", DataType.Utf8, s, None),
                  ("p", DataType.Float64, np.array(p), None)])


HAGG = [("MIN", 1), ("MAX", 1), ("COUNT", 1)]


@pytest.mark.parametrize("batch_rows", [0, 3])
def test_utf8_hand_built_strings(batch_rows):
    t = hand_table()
    some = BinaryExpr(Column(2), Operator.Gt, Literal(Float64(0.25)))
    none = BinaryExpr(Column(2), Operator.Gt, Literal(Float64(9.0)))
    for keys in (None, [0]):
        res = srun(t, None, keys, HAGG, batch_rows)
        scheck(t, None, None, keys, HAGG, res)
        scheck(t, some, t.values[2] > 0.25, keys, HAGG, srun(t, some, keys, HAGG, batch_rows))
    got, vs = srun(t, None, None, HAGG, batch_rows)
    assert (vs[0], vs[1]) == ([b""], [b"\xff"]) and (int(got[0].bits), int(got[1].bits)) == (0, 1)
    (dk, dv, _), vs = srun(t, None, [0], HAGG, batch_rows)
    assert vs[0] == [b"", b"aaaaaaaa", b"", None] and vs[1] == [b"\xff", b"aaaaaaaab", b"", None]
    assert [int(v[0].is_null) for v in dv] == [0, 0, 0, 1] and int(dv[2][0].count) == 1
    # a predicate that selects nothing: null, ungrouped; no group at all, grouped
    got, vs = srun(t, none, None, HAGG, batch_rows)
    assert (int(got[0].is_null), int(got[0].count), int(got[0].type), vs[0]) == (1, 0, UTF8, [None])
    (dk, dv, _), vs = srun(t, none, [0], HAGG, batch_rows)
    assert len(dk) == 0 and vs[0] == []


def test_utf8_long_strings_and_raw_null_slots():
    a, b = b"c" * 299 + b"x", b"c" * 299 + b"y"
    t = Table([("s", DataType.Utf8, [a, b, a, b, a], None), ("p", DataType.Float64, np.ones(5), None)])
    (got, vs) = srun(t, None, None, [("MIN", 0), ("MAX", 0)])
    assert vs == {0: [a], 1: [b]} and [int(v.bits) for v in got] == [300, 300]
    # a null slot holding non-empty bytes: not counted; after a Selection it counts with its raw bytes
    t = with_raw_nulls(Table([("s", DataType.Utf8, [b"m", b"zz", b"n", b"A"], None),
                              ("p", DataType.Float64, np.ones(4), None)]), 0, [True, False, True, False])
    two = [("MIN", 0), ("MAX", 0)]
    res = srun(t, None, None, two)
    scheck(t, None, None, None, two, res)
    assert res[1] == {0: [b"m"], 1: [b"n"]}
    allp = BinaryExpr(Column(1), Operator.Gt, Literal(Float64(0.0)))
    res = srun(t, allp, None, two)
    scheck(t, allp, np.ones(4, bool), None, two, res)
    assert res[1] == {0: [b"A"], 1: [b"zz"]} and int(res[0][0].count) == 4


# -------------------------------------------------------------------- random
@functools.lru_cache(maxsize=None)
def stable(ngroups: int, n: int = 3000) -> Table:
    """n rows, 20% nulls; strings of length 0-20 over {0x00, a, 0x80, 0xff}
    (many ties run past 8 bytes); Int64 and Utf8 keys of ~ngroups values."""
    rng = np.random.default_rng(7 + ngroups + n)
    alpha = np.array([0x00, 0x61, 0x80, 0xff], np.uint8)

    def strings(null_p):
        out = []
        for ln in rng.integers(0, 21, n):
            out.append(None if rng.random() < null_p else bytes(alpha[rng.integers(0, 4, int(ln))]))
        return out
    k = rng.integers(0, ngroups, n)
    words = [b"key-%d" % i if i % 3 else b"k\xff%d" % i for i in range(ngroups)]
    return Table([("k", DataType.Int64, k * 1_000_003 - 5_000_000, None),
                  ("ks", DataType.Utf8, [words[i] for i in k], None),
                  ("s", DataType.Utf8, strings(0.2), None), ("s2", DataType.Utf8, strings(0.2), None),
                  ("v", DataType.Int32, rng.integers(-1000, 1000, n).astype(np.int32), rng.random(n) >= 0.1),
                  ("b", DataType.Boolean, rng.random(n) < 0.5, rng.random(n) >= 0.2),
                  ("p", DataType.Float64, rng.random(n), None)])


SAGG = [("MIN", 2), ("MAX", 2), ("MIN", 3), ("COUNT", 2), ("SUM", 4), ("MIN", 5), ("MAX", 5)]
SPRED = BinaryExpr(Column(6), Operator.Lt, Literal(Float64(0.5)))


@pytest.mark.parametrize("batch_rows", [0, 64, 1000])
def test_utf8_random_ungrouped(batch_rows):
    t = stable(7)
    scheck(t, None, None, None, SAGG, srun(t, None, None, SAGG, batch_rows))
    scheck(t, SPRED, t.values[6] < 0.5, None, SAGG, srun(t, SPRED, None, SAGG, batch_rows))


@pytest.mark.parametrize("keys", [[0], [1], [0, 1]], ids=["int64", "utf8", "int64_utf8"])
@pytest.mark.parametrize("ngroups", [1, 7, 300])
def test_utf8_random_grouped(ngroups, keys):
    t = stable(ngroups)
    for batch_rows in (0, 64, 1000):
        scheck(t, None, None, keys, SAGG, srun(t, None, keys, SAGG, batch_rows))
    scheck(t, SPRED, t.values[6] < 0.5, keys, SAGG, srun(t, SPRED, keys, SAGG, 1000))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_utf8_small_row_counts(n):
    t = stable(7, n)
    scheck(t, None, None, None, SAGG, srun(t, None, None, SAGG))
    scheck(t, None, None, [0], SAGG, srun(t, None, [0], SAGG))


def test_utf8_row_order_does_not_matter():
    """Sorted ascending and descending by s, in 64-row batches: one order
    replaces the winner in every batch, the other never does."""
    t = stable(7)
    order = sorted(range(t.n), key=lambda i: (t.values[2][i] is None, t.values[2][i] or b""))

    def permuted(idx):
        return Table([(nm, ty, [v[i] for i in idx] if ty == DataType.Utf8 else np.asarray(v)[idx],
                       None if ty == DataType.Utf8 else t.valid[c][idx])
                      for c, (nm, ty, v) in enumerate(zip(t.names, t.types, t.values))])
    up, down = permuted(order), permuted(order[::-1])
    for keys in (None, [0]):
        a, b = srun(up, None, keys, SAGG[:4], 64), srun(down, None, keys, SAGG[:4], 64)
        ssame(a, b)
        scheck(up, None, None, keys, SAGG[:4], a)


# --------------------------------------------------- finishes, paths, growth
def _state(t, keys, aggs):
    s = t.schema
    cs = [compile_expr(None, a, s, SFL) for a in exprs(t, aggs)]
    eng = engine()
    st = eng.agg_state(cs) if keys is None else eng.grouped_agg_state(
        [compile_scalar_expr(None, Column(k), s, SFL) for k in keys], cs)
    return st, cs


def test_utf8_finish_then_more_reset_and_reuse():
    from test_gpu_aggregate import slice_batch
    t = stable(7)
    for keys in (None, [0]):
        st, cs = _state(t, keys, SAGG)
        dev = t.batch.to(engine().device)
        fin = collect(t, keys, SAGG)
        st.add(None, slice_batch(dev, 0, 1_003), SFL)   # (1_003: an arrow slice follows, offset 1_003)
        first = fin(st, cs)
        scheck(t.rows(0, 1_003), None, None, keys, SAGG, first)
        for r0 in range(1_003, t.n, 500):
            st.add(None, slice_batch(dev, r0, min(500, t.n - r0)), SFL)
        scheck(t, None, None, keys, SAGG, fin(st, cs))
        st.reset()
        st.add(None, slice_batch(dev, 0, 1_003), SFL)
        ssame(first, fin(st, cs))


def test_utf8_forced_paths(monkeypatch):
    t = stable(300)
    base = srun(t, None, [0, 1], SAGG, 1000)
    scheck(t, None, None, [0, 1], SAGG, base)
    monkeypatch.setenv("DFMI_DIAG", "1")
    for knob, value in (("DFMI_GROUP_BUCKETS", "0"), ("DFMI_GROUP_BUCKETS", "1"), ("DFMI_GROUP_HASH_BITS", "3"),
                        ("DFMI_GROUP_HOST", "1"), ("DFMI_GROUP_HOST_FINISH", "1")):
        monkeypatch.setenv(knob, value)
        before = _bucketed_batches()
        ssame(base, srun(t, None, [0, 1], SAGG, 1000))
        if knob == "DFMI_GROUP_BUCKETS":
            assert (_bucketed_batches() > before) == (value == "1")
        monkeypatch.delenv(knob)


@pytest.mark.parametrize("knob,value", [("DFMI_GROUP_HOST_FINISH", "1"), ("DFMI_GROUP_HASH_BITS", "3"),
                                        ("DFMI_GROUP_HOST", "1"), ("DFMI_GROUP_BUCKETS", "1")])
@pytest.mark.parametrize("keys", [[0], [0, 1]], ids=["int64", "int64_utf8"])
def test_utf8_forced_paths_few_groups(monkeypatch, knob, value, keys):
    """7 groups: the finish's first call has room for every group, so a finish
    that drains the device table (the host finish; rows the host merged beside
    the table's) produces its values in that one call -- and the bytes of
    every group's extremes must be there to ask for afterwards."""
    t = stable(7)
    base = srun(t, None, keys, SAGG, 1000)
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv(knob, value)
    res = srun(t, None, keys, SAGG, 1000)
    assert len(res[0][0]) == 7 and all(len(v) == 7 for v in res[1].values())
    scheck(t, None, None, keys, SAGG, res)
    ssame(base, res)
    # a finish, more batches, a finish again on the same path
    from test_gpu_aggregate import slice_batch
    st, cs = _state(t, keys, SAGG)
    dev = t.batch.to(engine().device)
    fin = collect(t, keys, SAGG)
    st.add(None, slice_batch(dev, 0, 1_000), SFL)
    scheck(t.rows(0, 1_000), None, None, keys, SAGG, fin(st, cs))
    st.add(None, slice_batch(dev, 1_000, t.n - 1_000), SFL)
    ssame(base, fin(st, cs))


def test_utf8_raw_null_slots_grouped():
    """Null slots holding non-empty bytes, in 3 groups: without a predicate
    they do not count; after a Selection the evaluation pass compacts the raw
    slot bytes and they count (and win) like any value."""
    s = [b"m", b"zz", b"n", b"A", b"q", b"!", b"r", b"~~~~~~~~~", b"c", b"b", b"a", b"aaaaaaaaZ"]
    valid = [True, False, True, False, True, False, True, False, False, False, False, True]
    k = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    p = [1.0] * 11 + [0.0]
    t = with_raw_nulls(Table([("k", DataType.Int64, np.array(k), None), ("s", DataType.Utf8, s, None),
                              ("p", DataType.Float64, np.array(p), None)]), 1, valid)
    for batch_rows in (0, 5):
        res = srun(t, None, [0], HAGG, batch_rows)
        scheck(t, None, None, [0], HAGG, res)
        assert res[1] == {0: [b"m", b"q", b"aaaaaaaaZ"], 1: [b"n", b"r", b"aaaaaaaaZ"]}
        some = BinaryExpr(Column(2), Operator.Gt, Literal(Float64(0.5)))
        res = srun(t, some, [0], HAGG, batch_rows)
        scheck(t, some, np.array(p) > 0.5, [0], HAGG, res)
        assert res[1] == {0: [b"A", b"!", b"a"], 1: [b"zz", b"~~~~~~~~~", b"c"]}
        assert [int(v[0].count) for v in res[0][1]] == [4, 4, 3]


def test_utf8_growth_many_groups():
    """~48,000 groups in 20,000-row batches: more than half the first
    65,536-slot table, which is grown and rehashed, and the records and the
    side arrays grow with it (1,024 at first); group ids stay stable, so every
    group's extreme is still its own."""
    rng = np.random.default_rng(5)
    n = 80_000
    k = rng.integers(0, 70_000, n)
    s = [bytes(rng.integers(97, 100, int(ln)).astype(np.uint8)) for ln in rng.integers(0, 12, n)]
    t = Table([("k", DataType.Int64, k, None), ("s", DataType.Utf8, s, None)])
    res = srun(t, None, [0], HAGG, 20_000)
    assert len(res[0][0]) > 40_000
    scheck(t, None, None, [0], HAGG, res)


@pytest.mark.parametrize("host", [False, True], ids=["device_batches", "host_batches"])
def test_utf8_coalesced_forms(host):
    t = stable(7)
    for keys in (None, [0], [1]):
        one = srun(t, None, keys, SAGG, 257)
        ssame(one, srun(t, None, keys, SAGG, 257, many=True, host=host))
        scheck(t, None, None, keys, SAGG, one)


def test_utf8_sql_relation_and_sort():
    from datafusion_amd.execution.sort import SortRelation
    from datafusion_amd.logicalplan import SortExpr
    from test_gpu_aggregate import slice_batch
    t = stable(7)
    fl = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY | _abi.DFMI_FLAG_EXT_SORT
    dev = t.batch.to(engine().device)
    batches = [slice_batch(dev, r0, min(64, t.n - r0)) for r0 in range(0, t.n, 64)]
    want = {}
    for i in range(t.n):
        if t.values[2][i] is not None:
            want.setdefault(int(t.values[0][i]), []).append(t.values[2][i])
    ks = sorted(want)
    for coalesce in (1, 256):
        ctx = ExecutionContext(flags=fl)
        ctx.register_datasource("t", MemoryDataSource(t.schema, list(batches)))
        rel = ctx.sql("SELECT k, MIN(s), MAX(s) FROM t GROUP BY k")
        assert isinstance(rel, AggregateRelation)
        rel.coalesce = coalesce
        srt = SortRelation(rel, [SortExpr(Column(1), False)], rel.schema(), None, fl, None, ctx)
        (rb,) = list(srt)
        assert [f.data_type for f in rb.schema.fields] == [DataType.Int64, DataType.Utf8, DataType.Utf8]
        rows = list(zip(rb.columns[0].to_pylist(), rb.columns[1].numpy_values(), rb.columns[2].numpy_values()))
        assert sorted(rows) == [(k, min(want[k]), max(want[k])) for k in ks]
        assert [r[1] for r in rows] == sorted((min(want[k]) for k in ks), reverse=True)
    ctx = ExecutionContext(flags=fl)
    ctx.register_datasource("t", MemoryDataSource(t.schema, list(batches)))
    out = ctx.sql("SELECT MIN(s), MAX(s2) FROM t").next()
    assert out.columns[0].numpy_values() == [min(x for x in t.values[2] if x is not None)]
    assert out.columns[1].numpy_values() == [max(x for x in t.values[3] if x is not None)]


# ------------------------------------------------------------ fixtures (Utf8)
@pytest.mark.parametrize("batch_rows", [0, 64])
def test_utf8_reference_fixture_cells(batch_rows):
    """csv_aggregate_all_types.csv cell 24 (MIN(c11); cell 25 is the
    reference's defect: MAX(c11) is checked against Python's maximum) and
    csv_aggregate_by_c_bool.csv cells 21 and 22 of both rows."""
    from golden_cases import all_types_typed, expected_rows, load_batch
    from test_gpu_aggregate import slice_batch
    schema = all_types_typed()
    batch = load_batch(schema, "all_types_flat.csv", has_header=True)
    c0, c11 = batch.columns[0].to_pylist(), batch.columns[11].numpy_values()
    dev = batch.to(engine().device)
    step = batch_rows or batch.num_rows()
    batches = [slice_batch(dev, r0, min(step, batch.num_rows() - r0)) for r0 in range(0, batch.num_rows(), step)]
    fl = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY
    ctx = ExecutionContext(flags=fl)
    ctx.register_datasource("t", MemoryDataSource(schema, list(batches)))
    out = ctx.sql("SELECT MIN(c11), MAX(c11) FROM t").next()
    (row,) = expected_rows("csv_aggregate_all_types.csv")
    assert out.columns[0].numpy_values() == [row[24].encode()] == [min(c11)]
    assert out.columns[1].numpy_values() == [max(c11)]
    ctx.register_datasource("t", MemoryDataSource(schema, list(batches)))
    (rb,) = list(ctx.sql("SELECT c0, MIN(c11), MAX(c11) FROM t GROUP BY c0"))
    rows = expected_rows("csv_aggregate_by_c_bool.csv")
    assert rb.columns[0].to_pylist() == [False, True] and len(rows) == 2
    for g, r in enumerate(rows):
        mine = [s for b, s in zip(c0, c11) if b == bool(g)]
        assert rb.columns[1].numpy_values()[g] == r[21].encode() == min(mine)
        assert rb.columns[2].numpy_values()[g] == r[22].encode() == max(mine)


# ------------------------------------------------- entry point, partials, arena
def test_utf8_value_bytes_entry_point():
    import ctypes as C
    t = hand_table()
    L = _abi.lib()
    for keys in (None, [0]):
        st, cs = _state(t, keys, HAGG)
        err, ln = _abi.dfmi_error(), C.c_int64(-1)
        offs, data = np.full(8, -7, np.int32), np.full(1024, 0xEE, np.uint8)
        call = lambda j, cap: L.dfmi_agg_state_value_bytes(st.handle, j, offs.ctypes.data, offs.size, data.ctypes.data, cap,  # noqa: E731
                                                           C.byref(ln), C.byref(err))
        assert call(1, 1024) == _abi.DFMI_ERR_INVALID_ARGUMENT and ln.value == 0   # no finish yet
        st.add(None, t.batch.to(engine().device), SFL)
        st.finish()
        for j in (-1, 2, 3):                                                       # out of range, a COUNT
            assert call(j, 1024) == _abi.DFMI_ERR_INVALID_ARGUMENT
        ln.value = -1
        assert call(1, 0) == _abi.DFMI_ERR_CAPACITY                                # too small: the length, nothing written
        assert ln.value == (1 if keys is None else 1 + 9 + 0) and (offs == -7).all() and (data == 0xEE).all()
        assert call(1, 1024) == _abi.DFMI_OK
        rows = 1 if keys is None else 4
        assert offs[0] == 0 and offs[rows] == ln.value
        if keys is not None:
            assert list(offs[:5]) == [0, 1, 10, 10, 10]                            # "" and the null group: empty slots
            assert bytes(data[:10]) == b"\xffaaaaaaaab"


def test_utf8_partials_are_refused():
    t = stable(7)
    msg = "partial state of a Utf8 MIN / MAX aggregate"
    comm = ShardComm(engine(), 1, 0, ShardComm.unique_id())
    for keys, finish in ((None, lambda st: st.partial()), ([0], lambda st: st.partial()),
                         (None, lambda st: comm.agg_finish(st)), ([0], lambda st: comm.agg_finish_grouped(st))):
        st, cs = _state(t, keys, SAGG)
        st.add(None, t.batch.to(engine().device), SFL)
        with pytest.raises(ExecutionError) as ei:
            finish(st)
        assert (ei.value.kind, ei.value.message) == ("NotImplemented", msg)
    # Boolean extremes beside them go through partials in a state without a Utf8 extreme
    st, cs = _state(t, None, [("MIN", 5), ("MAX", 5)])
    st.add(None, t.batch.to(engine().device), SFL)
    same(merge_agg_partials(cs, [st.partial()]), st.finish())


def test_utf8_arena_stays_bounded():
    """200 descending 64-row batches over 50 groups (every batch replaces every
    group's MIN winner, so superseded strings pile up unless the arena is
    compacted): the reserved arena bytes after batch 200 are those after
    batch 50."""
    import ctypes as C
    from test_gpu_aggregate import slice_batch
    L = _abi.lib()
    L.dfmi_internal_agg_str_arena_bytes.argtypes = [C.c_void_p]
    L.dfmi_internal_agg_str_arena_bytes.restype = C.c_longlong
    n = 200 * 64
    s = [b"%06d-%s" % (n - i, b"x" * 40) for i in range(n)]   # descending: each row beats the ones before it
    k = np.arange(n) % 50
    t = Table([("k", DataType.Int64, k, None), ("s", DataType.Utf8, s, None)])
    st, cs = _state(t, [0], [("MIN", 1), ("MAX", 1)])
    dev = t.batch.to(engine().device)
    reserved = []
    for b in range(200):
        st.add(None, slice_batch(dev, b * 64, 64), SFL)
        reserved.append(L.dfmi_internal_agg_str_arena_bytes(st.handle))
    assert reserved[49] > 0 and reserved[199] == reserved[49]
    fin = collect(t, [0], [("MIN", 1), ("MAX", 1)])
    scheck(t, None, None, [0], [("MIN", 1), ("MAX", 1)], fin(st, cs))
