"""GPU tests of the Utf8 ordering comparisons (DFMI_FLAG_EXT_UTF8_ORDER with
DFMI_FLAG_EXT_UTF8_COMPARE): <, <=, >, >= over Utf8 operands, bytewise and
unsigned, a proper prefix first, nulls by arrow's cmp_opt.

The oracle executes no Utf8 comparison, so expected values never come from
the device and never from the oracle's view of such a node: `lower` replaces
every Utf8 ordering node by a Column over a non-nullable Boolean array that
this file computes from the host batch -- Python's bytes order for valid
pairs, the cmp_opt table written out for nulls -- and the lowered query runs
through the oracle with the remaining flags. A Selection drops validity
(filter.rs:84-93), so a query that compares Utf8 after one is expected in two
steps: the oracle's filter of every column, then the projections lowered over
that all-valid batch (a null slot then compares by its raw bytes)."""
import os

import numpy as np
import pytest
import torch

from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema, pack_bits
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.engine import engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator, Utf8
from datafusion_amd.sqlplanner import SqlToRel
from oracle_ffi import oracle_aggregate_grouped, oracle_filter_project
from test_gpu_parity import assert_same
from test_gpu_sort import pull_all

pytestmark = pytest.mark.gpu

CMP, ORD = _abi.DFMI_FLAG_EXT_UTF8_COMPARE, _abi.DFMI_FLAG_EXT_UTF8_ORDER
FL = CMP | ORD
ORDER_OPS = [Operator.Lt, Operator.LtEq, Operator.Gt, Operator.GtEq]
U8, F64, BOOL = DataType.Utf8, DataType.Float64, DataType.Boolean


def lit(b: bytes) -> Literal:
    return Literal(Utf8(b.decode("utf-8", errors="surrogateescape")))


def lit_bytes(e: Literal) -> bytes:
    return e.value.value.encode("utf-8", errors="surrogateescape")


# ------------------------------------------------------------ the restatement
def order_values(op, a, b):
    """a OP b over two lists of bytes (Python's bytes order is the contract's)."""
    f = {Operator.Lt: lambda x, y: x < y, Operator.LtEq: lambda x, y: x <= y,
         Operator.Gt: lambda x, y: x > y, Operator.GtEq: lambda x, y: x >= y}[op]
    return np.fromiter((f(x, y) for x, y in zip(a, b)), bool, len(a))


def cmp_opt(op, lv, rv, res):
    """arrow's cmp_opt as the numeric comparisons apply it: never null; a null
    is less than every value; null against null: Lt / LtEq true, Gt / GtEq false."""
    either_null = lv if op in (Operator.Gt, Operator.GtEq) else ~lv
    return np.where(lv & rv, res, either_null)


def is_utf8(e, schema):
    return (isinstance(e, Literal) and e.value.dtype == U8) or \
        (isinstance(e, Column) and schema.fields[e.index].data_type == U8)


def operand(e, batch, words):
    """(values, valid) of a Utf8 operand; `words` = {column: (dictionary, index)}
    lets a large column be compared per dictionary word."""
    n = batch.num_rows()
    if isinstance(e, Literal):
        return [lit_bytes(e)] * n, np.ones(n, bool)
    a = batch.columns[e.index]
    return a.numpy_values(), a.valid_mask()


def order_node(e, batch, words):
    l, r = e.left, e.right
    n = batch.num_rows()
    for col, other, flip in ((l, r, False), (r, l, True)):
        if isinstance(col, Column) and isinstance(other, Literal) and words and col.index in words:
            d, idx = words[col.index]  # per word, then indexed
            q = [lit_bytes(other)] * len(d)
            res = order_values(e.op, q, d)[idx] if flip else order_values(e.op, d, q)[idx]
            v = batch.columns[col.index].valid_mask()
            return cmp_opt(e.op, np.ones(n, bool), v, res) if flip else cmp_opt(e.op, v, np.ones(n, bool), res)
    (a, av), (b, bv) = operand(l, batch, words), operand(r, batch, words)
    return cmp_opt(e.op, av, bv, order_values(e.op, a, b))


def lower(e, schema, batch, words=None):
    """e with every Utf8 ordering node replaced by a Boolean Column: (e', schema', batch')."""
    if isinstance(e, BinaryExpr):
        if e.op in ORDER_OPS and is_utf8(e.left, schema) and is_utf8(e.right, schema):
            arr = Array.from_numpy(BOOL, order_node(e, batch, words))
            s2 = Schema(list(schema.fields) + [Field("_o%d" % len(schema.fields), BOOL, False)])
            return Column(len(schema.fields)), s2, RecordBatch(s2, list(batch.columns) + [arr])
        l, schema, batch = lower(e.left, schema, batch, words)
        r, schema, batch = lower(e.right, schema, batch, words)
        return BinaryExpr(l, e.op, r), schema, batch
    return e, schema, batch


def expected(schema, batch, pred, projs, flags=FL, words=None):
    """Projection(Selection?(batch)) as Arrays (or the oracle's ExecutionError)."""
    s, b = schema, batch
    if pred is not None:
        p, s2, b2 = lower(pred, schema, batch, words)
        # (the oracle's Selection filters every column, the appended Boolean ones too: GATHER_ALL)
        cols = oracle_filter_project(s2, b2, p, [Column(i) for i in range(len(schema.fields))],
                                     (flags & ~ORD) | _abi.DFMI_FLAG_EXT_GATHER_ALL)
        if all(isinstance(e, Column) for e in projs):
            return [cols[e.index][1] for e in projs]
        s = Schema([Field(f.name, f.data_type, False) for f in schema.fields])
        b = RecordBatch(s, [a for _, a in cols])
        words = None  # the filtered batch is compared row by row
    out = []
    for e in projs:
        e2, s2, b2 = lower(e, s, b, words)
        out.append(oracle_filter_project(s2, b2, None, [e2], flags & ~ORD)[0][1])
    return out


def programs(schema, pred, projs, flags=FL):
    return (compile_scalar_expr(None, pred, schema, flags) if pred is not None else None,
            [compile_scalar_expr(None, e, schema, flags) for e in projs])


def check(schema, batch, pred, projs, flags=FL, words=None, host=True, what=""):
    """Device, host and chunked-host results against the expectation."""
    want = expected(schema, batch, pred, projs, flags, words)
    p, cp = programs(schema, pred, projs, flags)
    runs = [("device", lambda: [a.cpu() for a in engine().filter_project(p, cp, batch, flags)])]
    if host:
        def chunked():
            os.environ["DFMI_HOST_CHUNK_ROWS"] = "1024"
            try:
                return engine().filter_project_host(p, cp, batch, flags)
            finally:
                del os.environ["DFMI_HOST_CHUNK_ROWS"]
        runs += [("host", lambda: engine().filter_project_host(p, cp, batch, flags)), ("chunked host", chunked)]
    for name, run in runs:
        got = run()
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, "%s %s: %r col %d" % (what, name, pred, j))
    return want


# -------------------------------------------------------------------- the data
L40 = bytes(97 + i % 23 for i in range(40))
L200 = bytes(97 + i % 23 for i in range(200))
L300 = bytes(97 + i % 23 for i in range(300))


def near(l):
    """l but for its last byte, both ways."""
    return [l[:-1] + bytes([l[-1] - 1]), l[:-1] + b"\x80"]


DICT = [b"", b"a", b"a\0", b"a\0\0", b"ab", b"abc", b"abcd", b"abcde", b"abcdefg", b"abcdefgh", b"abcdefghi",
        b"abcdefgh\x7f", b"abcdefgh\x80", b"abcdefgh\x80z", b"abcdefgh\xff", b"\xff", b"\xe2\x82\xac uro",
        L40, L300, L200, L200[:-1], L200 + b"\0", L40[:-1], L40 + b"a"] + near(L40) + near(L300) + near(L200)
LITERALS = [b"", b"a", b"abcd", b"abcde", b"abcdefgh", b"abcdefghi", b"abcdefgh\x80", L40, L200]


def raw_utf8(strings, valid):
    """A Utf8 Array built directly: null slots keep their bytes."""
    offs = np.zeros(len(strings) + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in strings])
    data = np.frombuffer(b"".join(strings), np.uint8).copy()
    nulls = int(len(strings) - valid.sum())
    return Array(U8, len(strings), torch.from_numpy(data), torch.from_numpy(pack_bits(valid)) if nulls else None,
                 torch.from_numpy(offs), nulls)


S3 = Schema([Field("s", U8, True), Field("t", U8, False), Field("v", F64, True)])
_table = {}


def table(n=5000):
    """s: ~10% nulls whose slots span bytes; t: no nulls; v in [0, 1), ~10% nulls. Built once."""
    if n not in _table:
        rng = np.random.default_rng(71)
        s = [DICT[i] for i in rng.integers(0, len(DICT), n)]
        t = [DICT[i] for i in rng.integers(0, len(DICT), n)]
        sv = rng.random(n) >= 0.1
        assert sum(len(x) for x, ok in zip(s, sv) if not ok) > 1000
        _table[n] = RecordBatch(S3, [raw_utf8(s, sv), raw_utf8(t, np.ones(n, bool)),
                                     Array.from_numpy(F64, rng.random(n), rng.random(n) >= 0.1)])
    return _table[n]


# ----------------------------------------------------- 1. one tile with a tail
@pytest.mark.parametrize("op", ORDER_OPS, ids=[o.name for o in ORDER_OPS])
def test_every_operator_against_the_literals_both_sides(op):
    b = table()
    for q in LITERALS:
        # rows equal to the literal, a proper prefix of it (but for ""), an extension of it
        assert q in DICT and (q == b"" or any(w != q and q.startswith(w) for w in DICT)) and \
            any(w != q and w.startswith(q) for w in DICT)
        for pred in (BinaryExpr(Column(0), op, lit(q)), BinaryExpr(lit(q), op, Column(0))):
            want = check(S3, b, pred, [Column(0), Column(2)], host=q in (b"abcd", b"abcdefghi", L200), what=repr(q))
            assert q == b"" or 0 < want[0].length < b.num_rows()


@pytest.mark.parametrize("op", ORDER_OPS, ids=[o.name for o in ORDER_OPS])
def test_column_against_column(op):
    b = table()
    both = Schema([Field("s", U8, True), Field("t", U8, True), Field("v", F64, True)])
    rng = np.random.default_rng(72)
    tv = rng.random(b.num_rows()) >= 0.1
    t2 = raw_utf8(b.columns[1].numpy_values(), tv)
    b2 = RecordBatch(both, [b.columns[0], t2, b.columns[2]])
    assert ((~b.columns[0].valid_mask()) & ~tv).sum() > 10  # null against null
    for sch, bb in ((S3, b), (both, b2)):
        for pred in (BinaryExpr(Column(0), op, Column(1)), BinaryExpr(Column(1), op, Column(0))):
            want = check(sch, bb, pred, [Column(0), Column(1)])
            assert 0 < want[0].length < bb.num_rows()


# ------------------------------------------- 2. projection and mixed predicate
V_LT = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5)))


def test_projection_unfiltered_and_after_a_selection():
    b = table()
    projs = [BinaryExpr(Column(0), Operator.Lt, lit(b"abcd")), Column(0), BinaryExpr(lit(L40), Operator.GtEq, Column(0)),
             BinaryExpr(Column(0), Operator.LtEq, Column(1)), BinaryExpr(lit(b"a"), Operator.Lt, lit(b"a\0"))]
    want = check(S3, b, None, projs)
    assert want[0].data_type == BOOL and want[0].null_count == 0 and 0 < want[0].numpy_values().sum() < b.num_rows()
    assert want[4].numpy_values().all()
    # after WHERE v < 0.5 the columns are all-valid: the null slots' bytes are compared
    two = check(S3, b, V_LT, projs)
    sel = np.flatnonzero(expected(S3, b, None, [V_LT])[0].numpy_values())
    one_step = want[0].numpy_values()[sel]
    assert two[0].length == len(sel) and (two[0].numpy_values() != one_step).sum() > 10


def test_mixed_and_range_predicates():
    b = table()
    mixed = BinaryExpr(V_LT, Operator.And, BinaryExpr(Column(0), Operator.GtEq, lit(b"abc")))
    rng_ = BinaryExpr(BinaryExpr(Column(0), Operator.GtEq, lit(b"ab")), Operator.And,
                      BinaryExpr(Column(0), Operator.Lt, lit(b"ac")))
    for pred in (mixed, rng_):
        want = check(S3, b, pred, [Column(0), Column(2), BinaryExpr(Column(1), Operator.Gt, lit(b"abcdefgh"))])
        assert 100 < want[0].length < b.num_rows() - 100


def test_first_error_order_around_an_ordering_node():
    """A DivideByZero and a Utf8-against-Float64 "comparison_ops" on either
    side of an ordering node: the error the oracle raises for the lowered query."""
    b = table()
    v = np.array(b.columns[2].numpy_values()).copy()
    v[[1234, 4000]] = 0.0
    valid = b.columns[2].valid_mask().copy()
    valid[[1234, 4000]] = True
    bz = RecordBatch(S3, [b.columns[0], b.columns[1], Array.from_numpy(F64, v, valid)])
    ordn = BinaryExpr(Column(0), Operator.Lt, lit(b"abcde"))
    div = BinaryExpr(BinaryExpr(Literal(Float64(1.0)), Operator.Divide, Column(2)), Operator.Gt, Literal(Float64(1.5)))
    mismatch = BinaryExpr(Column(0), Operator.Lt, Column(2))
    kinds = set()
    for pred in (BinaryExpr(BinaryExpr(ordn, Operator.And, div), Operator.And, mismatch),
                 BinaryExpr(BinaryExpr(mismatch, Operator.And, ordn), Operator.And, div),
                 BinaryExpr(ordn, Operator.And, div)):
        with pytest.raises(ExecutionError) as ref:
            expected(S3, bz, pred, [Column(0)])
        p, cp = programs(S3, pred, [Column(0)])
        with pytest.raises(ExecutionError) as dev:
            engine().filter_project(p, cp, bz, FL)
        assert (dev.value.kind, dev.value.message) == (ref.value.kind, ref.value.message)
        kinds.add(ref.value.kind)
    assert len(kinds) == 2
    # without DFMI_FLAG_EXT_UTF8_ORDER the ordering node itself is "comparison_ops", as before
    p, cp = programs(S3, ordn, [Column(0)], CMP)
    with pytest.raises(ExecutionError) as dev:
        engine().filter_project(p, cp, b, CMP)
    assert (dev.value.kind, dev.value.message) == ("ExecutionError", "comparison_ops")


# --------------------------------------------------------------- 3. many tiles
S2 = Schema([Field("s", U8, True), Field("v", F64, True)])


def word_table(n, seed, max_len=70, nwords=300, null_frac=0.05, pad=0):
    """Dictionary-coded Utf8 column built with numpy; `pad` bytes in front of the byte buffer."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(0, max_len + 1))).astype(np.uint8)) for _ in range(nwords)]
    idx = rng.integers(0, nwords, n)
    wl = np.array([len(w) for w in words])
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(wl[idx])
    wo = np.zeros(nwords + 1, np.int64)
    wo[1:] = np.cumsum(wl)
    dict_bytes = np.frombuffer(b"".join(words), np.uint8)
    pos = np.arange(offs[-1]) - np.repeat(offs[:-1], wl[idx]) + np.repeat(wo[idx], wl[idx])
    flat = dict_bytes[pos]
    valid = rng.random(n) >= null_frac
    v = Array.from_numpy(F64, rng.random(n), rng.random(n) >= 0.1)
    return words, idx, flat, offs.astype(np.int32), valid, v


def test_many_tiles_ranges_and_misaligned_byte_base():
    n = 300_001
    words, idx, flat, offs, valid, v = word_table(n, 73)
    dev = engine().device
    vb, ot, nulls = torch.from_numpy(pack_bits(valid)), torch.from_numpy(offs), int(n - valid.sum())
    srt = sorted(words)
    half = (srt[75], srt[225])  # about half of the rows
    one = next(w for w in srt[150:] if len(w) > 8)  # one word of 300: ~0.3% ... and its successor bound
    preds = [BinaryExpr(BinaryExpr(Column(0), Operator.GtEq, lit(half[0])), Operator.And,
                        BinaryExpr(Column(0), Operator.Lt, lit(half[1]))),
             BinaryExpr(BinaryExpr(Column(0), Operator.GtEq, lit(one)), Operator.And,
                        BinaryExpr(Column(0), Operator.LtEq, lit(one + b"\0")))]
    want = {}
    for pad in (0, 1, 2, 3):
        big = torch.zeros(len(flat) + 8, dtype=torch.uint8)
        big[pad:pad + len(flat)] = torch.from_numpy(flat)
        host = RecordBatch(S2, [Array(U8, n, big[pad:pad + len(flat)], vb, ot, nulls), v])
        dbig = big.to(dev)
        assert dbig.data_ptr() % 4 == 0
        db = RecordBatch(S2, [Array(U8, n, dbig[pad:pad + len(flat)], vb.to(dev), ot.to(dev), nulls), v.to(dev)])
        for j, pred in enumerate(preds):
            if j not in want:  # the reference once
                want[j] = expected(S2, host, pred, [Column(0), Column(1)], words={0: (words, idx)})
                frac = want[j][0].length / n
                assert (0.3 < frac < 0.7) if j == 0 else (0 < frac < 0.01)
            p, cp = programs(S2, pred, [Column(0), Column(1)])
            got = engine().filter_project(p, cp, db, FL)
            for g, w in zip(got, want[j]):
                assert_same(g.cpu(), w, "pad %d pred %d" % (pad, j))


# ------------------------------------------------------------ 4. kernel switch
def test_high_selectivity_switches_to_the_one_tile_kernel():
    n = (1 << 22) + 5
    words, idx, flat, offs, valid, v = word_table(n, 74, max_len=24, null_frac=0.03)
    dev = engine().device
    nulls = int(n - valid.sum())
    host = RecordBatch(S2, [Array(U8, n, torch.from_numpy(flat), torch.from_numpy(pack_bits(valid)),
                                  torch.from_numpy(offs), nulls), v])
    db = host.to(dev)
    pred = BinaryExpr(Column(0), Operator.GtEq, lit(sorted(words)[len(words) // 2]))
    want = expected(S2, host, pred, [Column(0), Column(1)], words={0: (words, idx)})
    assert 0.3 < want[0].length / n < 0.7
    p, cp = programs(S2, pred, [Column(0), Column(1)])
    names = []
    for _ in range(2):
        got = engine().filter_project(p, cp, db, FL)
        names.append(_abi.lib().dfmi_last_kernel_name(engine().ctx))
        for g, w in zip(got, want):
            assert_same(g.cpu(), w, "s >= median word")
    assert names[0] != names[1]


# ------------------------------------------------------------ 5. small batches
RANGE_SQL = "SELECT s, v FROM t WHERE s >= 'w2' AND s < 'w3'"


def w_table(n, seed, null_frac=0.08):
    rng = np.random.default_rng(seed)
    s = [b"w%d" % i if i % 7 else b"w%dx\xc3\xa9" % i for i in rng.integers(0, 600, n)]
    sv = rng.random(n) >= null_frac
    return RecordBatch(S2, [raw_utf8(s, sv), Array.from_numpy(F64, rng.random(n), rng.random(n) >= 0.1)])


def plan_of(sql, schema, flags):
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(schema, []))
    return SqlToRel(ctx).sql_to_rel(sql)


def test_twenty_small_batches_coalesced():
    nb, rows = 20, 1024
    whole = w_table(nb * rows, 75)
    sv, vals = whole.columns[0].valid_mask().copy(), whole.columns[0].numpy_values()
    vals[3 * rows:4 * rows] = [b"x%d" % i for i in range(rows)]  # a batch that selects nothing
    sv[3 * rows:4 * rows] = True
    sv[5 * rows:6 * rows] = True                                  # a batch without nulls
    whole = RecordBatch(S2, [raw_utf8(vals, sv), whole.columns[1]])
    fv, fm = np.array(whole.columns[1].numpy_values()), whole.columns[1].valid_mask()
    batches = [RecordBatch(S2, [raw_utf8(vals[lo:lo + rows], sv[lo:lo + rows]),
                                Array.from_numpy(F64, fv[lo:lo + rows], fm[lo:lo + rows])])
               for lo in range(0, nb * rows, rows)]
    assert batches[5].columns[0].null_count == 0 and batches[6].columns[0].null_count > 0
    plan = plan_of(RANGE_SQL, S2, FL)
    want = expected(S2, whole, plan.input.expr, plan.expr)
    per = [expected(S2, b, plan.input.expr, plan.expr) for b in batches]
    assert per[3][0].length == 0 and sum(w[0].length for w in per) == want[0].length > 500
    # FilterRelation / ProjectRelation over host batches: one coalesced call
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(S2, batches))
    got = pull_all(ctx.sql(RANGE_SQL))
    assert len(got) == nb
    for i, (rb, w) in enumerate(zip(got, per)):
        for j in range(2):
            assert_same(rb.columns[j].cpu(), w[j], "host batch %d col %d" % (i, j))
    # ... and dfmi_filter_project_batches over device batches
    p, cp = programs(S2, plan.input.expr, plan.expr)
    res, err = engine().filter_project_batches(p, cp, [b.to(engine().device) for b in batches], FL)
    assert err is None and len(res) == nb
    for i, (cols, w) in enumerate(zip(res, per)):
        for j in range(2):
            assert_same(cols[j].cpu(), w[j], "device batch %d col %d" % (i, j))


# ---------------------------------------------------------------- 6. around it
def test_sql_prefix_range_and_serde_worker():
    b = w_table(700, 76)
    plan = plan_of(RANGE_SQL, S2, FL)
    want = expected(S2, b, plan.input.expr, plan.expr)
    assert 30 < want[0].length < 200
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(S2, [b.to(engine().device)]))
    (rb,) = pull_all(ctx.sql(RANGE_SQL))
    for g, w in zip(rb.columns, want):
        assert_same(g.cpu(), w, "ctx.sql")
    import pyarrow as pa
    ctx = ExecutionContext(flags=FL)  # (the first pull drained the source)
    ctx.register_datasource("t", MemoryDataSource(S2, [b.to(engine().device)]))
    t = pa.ipc.open_stream(serde.run_physical_plan(ctx, serde.to_json(serde.Interactive(plan)))).read_all()
    assert t.num_rows == want[0].length
    assert [x.encode() for x in t.column(0).to_pylist()] == want[0].numpy_values()
    m = want[1].valid_mask()
    assert np.array_equal(np.array(t.column(1).is_valid().to_pylist()), m)
    assert np.array_equal(t.column(1).to_numpy(zero_copy_only=False).view(np.uint64)[m],
                          np.array(want[1].numpy_values()).view(np.uint64)[m])


def test_sql_aggregate_over_an_ordering_filter():
    AGG = _abi.DFMI_FLAG_EXT_AGGREGATE
    n = 900
    rng = np.random.default_rng(77)
    s = [bytes(rng.integers(97, 123, int(rng.integers(0, 6))).astype(np.uint8)) for _ in range(n)]
    sch = Schema([Field("s", U8, True), Field("v", F64, True), Field("b", BOOL, False)])
    b = RecordBatch(sch, [raw_utf8(s, rng.random(n) >= 0.1), Array.from_numpy(F64, rng.random(n), rng.random(n) >= 0.1),
                          Array.from_numpy(BOOL, rng.random(n) < 0.5)])
    sql = "SELECT MIN(v), COUNT(v) FROM t WHERE s < 'm' GROUP BY b"
    flags = FL | AGG | _abi.DFMI_FLAG_EXT_GATHER_ALL  # (a Boolean column under a Selection)
    plan = plan_of(sql, sch, flags)
    pred = plan.input.expr
    assert repr(pred) == '#0 Lt Utf8("m")'
    lp, ls, lb = lower(pred, sch, b)
    rk, rv = oracle_aggregate_grouped(ls, lb, lp, Column(2), list(plan.aggr_expr), flags & ~ORD)
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(sch, [b.to(engine().device)]))
    (rb,) = pull_all(ctx.sql(sql))
    assert rb.num_rows() == len(rk) == 2
    cols = [c.cpu() for c in rb.columns]
    mins = np.array(cols[-2].numpy_values()).view(np.uint64)
    counts = np.array(cols[-1].numpy_values())
    for g in range(2):
        assert not rv[g][0].is_null and int(mins[g]) == rv[g][0].bits
        assert int(counts[g]) == rv[g][1].bits and rv[g][1].bits > 50


def test_order_by_limit_over_an_ordering_filter():
    flags = FL | _abi.DFMI_FLAG_EXT_SORT
    b = w_table(800, 78)
    sql = "SELECT s, v FROM t WHERE s >= 'w2' AND s < 'w3' ORDER BY v LIMIT 5"
    plan = plan_of(RANGE_SQL, S2, FL)
    want = expected(S2, b, plan.input.expr, plan.expr)
    m = want[1].valid_mask()
    v = np.array(want[1].numpy_values())
    assert m.sum() > 20 and len(np.unique(v[m])) == m.sum()
    order = np.flatnonzero(m)[np.argsort(v[m], kind="stable")][:5]  # ascending: nulls last
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(S2, [b.to(engine().device)]))
    (rb,) = pull_all(ctx.sql(sql))
    got_s, got_v = rb.columns[0].cpu(), rb.columns[1].cpu()
    assert got_s.length == 5 and got_v.null_count == 0
    assert got_s.numpy_values() == [want[0].numpy_values()[i] for i in order]
    assert np.array_equal(np.array(got_v.numpy_values()).view(np.uint64), v[order].view(np.uint64))
